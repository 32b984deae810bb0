// The key-walking attention family of attn_walk.h at HD = 88: OpenCLIP ViT-g/14's vision tower (width 1408 = 16 heads of 88; 257 tokens + prompts).  Nine
// kernels, an object of their own; called by lpi_attn_hd_fwd / _bwd (attn_hd.hip), which check the arguments.
#include "attn_walk.h"
#include "attn_hd_widths.h"

namespace {
inline WalkArgs walk_args(const AttnHdCall& c) { return WalkArgs{c.B, c.L, c.H, c.qkv, c.ldqkv, c.ctx, c.ldctx, c.dctx, c.lddctx, c.lse, c.delta, c.dqkv, c.lddqkv}; }
}  // namespace

int attn_hd88_fwd(int dtype, const AttnHdCall& c, hipStream_t s) { return walk_fwd<88>(dtype, walk_args(c), s); }
int attn_hd88_bwd(int dtype, const AttnHdCall& c, hipStream_t s) { return walk_bwd<88>(dtype, walk_args(c), s); }
