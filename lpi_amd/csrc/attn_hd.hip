// Multi-head attention for heads that are NOT 64 wide (non-causal, uniform sequences, 1 <= L <= 1024): the key-walking family of attn_walk.h at the widths
// that ship — 80 (OpenCLIP ViT-H/14's vision tower: width 1280 = 16 heads of 80; instantiated here), 88 (ViT-g/14: 1408 = 16 x 88; attn_hd88.hip) and 104
// (ViT-bigG/14: 1664 = 16 x 104; attn_hd104.hip); 257 tokens + prompts each.  The entry points below are the only ones: they check every argument and
// dispatch on head_dim.
//
// replaces: nn.MultiheadAttention of a vision tower whose width / heads != 64 (retrieval/models/clip/model.py:183-185 computes width // 64 heads and cannot
// build such a tower; open_clip's ViT-H-14 has head_width 80, ViT-g-14 88, ViT-bigG-14 104).
#include "attn_walk.h"
#include "attn_hd_widths.h"

namespace {

constexpr int HDW = 80;      // the width instantiated in this object

// the widths that are built, by list: 72 and 96 are multiples of 8 too and are not
inline bool hd_width_ok(int head_dim) { return head_dim == HDW || head_dim == 88 || head_dim == 104; }
inline bool hd_shape_ok(int L, int H, int head_dim) { return hd_width_ok(head_dim) && L > 0 && L <= 1024 && H > 0; }
// B H is the grid's y extent
inline bool hd_bad(int dtype, int B, int L, int H, int head_dim) {
    return (dtype != LPI_F32 && dtype != LPI_BF16 && dtype != LPI_F16) || !hd_shape_ok(L, H, head_dim) || B <= 0 || (long long)B * H > 65535;
}
inline bool hd_bad_ld(int ld, long long cols, int esz) { return ld < cols || ((long long)ld * esz) % 16 != 0; }

inline int hd_fwd(int head_dim, int dtype, const AttnHdCall& c, hipStream_t s) {
    switch (head_dim) {
        case HDW: return walk_fwd<HDW>(dtype, WalkArgs{c.B, c.L, c.H, c.qkv, c.ldqkv, c.ctx, c.ldctx, c.dctx, c.lddctx, c.lse, c.delta, c.dqkv, c.lddqkv}, s);
        case 88: return attn_hd88_fwd(dtype, c, s);
        case 104: return attn_hd104_fwd(dtype, c, s);
    }
    return LPI_EINVAL;
}
inline int hd_bwd(int head_dim, int dtype, const AttnHdCall& c, hipStream_t s) {
    switch (head_dim) {
        case HDW: return walk_bwd<HDW>(dtype, WalkArgs{c.B, c.L, c.H, c.qkv, c.ldqkv, c.ctx, c.ldctx, c.dctx, c.lddctx, c.lse, c.delta, c.dqkv, c.lddqkv}, s);
        case 88: return attn_hd88_bwd(dtype, c, s);
        case 104: return attn_hd104_bwd(dtype, c, s);
    }
    return LPI_EINVAL;
}

}  // namespace

extern "C" int lpi_attn_hd_supported(int L, int H, int head_dim) { return hd_shape_ok(L, H, head_dim) ? 1 : 0; }

extern "C" int lpi_attn_hd_fwd(int dtype, int B, int L, int H, int head_dim, const void* qkv, int ldqkv, void* ctx, int ldctx, float* lse, void* stream) {
    if (hd_bad(dtype, B, L, H, head_dim) || !qkv || !ctx || !lse) return LPI_EINVAL;
    const int esz = dtype == LPI_F32 ? 4 : 2;
    const long long d = (long long)H * head_dim;
    if (hd_bad_ld(ldqkv, 3 * d, esz) || ldctx < d || (ldctx & 7)) return LPI_EINVAL;
    if (((uintptr_t)qkv | (uintptr_t)ctx) & 15) return LPI_EINVAL;
    return hd_fwd(head_dim, dtype, AttnHdCall{B, L, H, qkv, ldqkv, ctx, ldctx, nullptr, 0, lse, nullptr, nullptr, 0}, (hipStream_t)stream);
}

extern "C" int lpi_attn_hd_bwd(int dtype, int B, int L, int H, int head_dim, const void* qkv, int ldqkv, const void* ctx, int ldctx, const void* dctx, int lddctx,
                               const float* lse, float* delta, void* dqkv, int lddqkv, void* stream) {
    if (hd_bad(dtype, B, L, H, head_dim) || !qkv || !ctx || !dctx || !lse || !delta || !dqkv) return LPI_EINVAL;
    const int esz = dtype == LPI_F32 ? 4 : 2;
    const long long d = (long long)H * head_dim;
    if (hd_bad_ld(ldqkv, 3 * d, esz) || hd_bad_ld(lddqkv, 3 * d, esz) || hd_bad_ld(ldctx, d, esz) || hd_bad_ld(lddctx, d, esz)) return LPI_EINVAL;
    if (((uintptr_t)qkv | (uintptr_t)ctx | (uintptr_t)dctx | (uintptr_t)dqkv) & 15) return LPI_EINVAL;
    return hd_bwd(head_dim, dtype, AttnHdCall{B, L, H, qkv, ldqkv, ctx, ldctx, dctx, lddctx, const_cast<float*>(lse), delta, dqkv, lddqkv}, (hipStream_t)stream);
}
