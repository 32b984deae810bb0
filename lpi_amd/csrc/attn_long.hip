// Multi-head attention for LONG sequences of 64-wide heads (288 < L <= 1024 tokens, non-causal, uniform): the key-walking family of attn_walk.h at HD = 64.
//
// replaces: nn.MultiheadAttention of the reference's vision tower (retrieval/models/clip/model.py:183-185) at the one CLIP ViT of clip.available_models()
// (clip.py:30-40) whose sequences do not fit the one-workgroup-per-(sample, head) kernels of attention.hip / attention4.hip: ViT-L/14@336px, 577 tokens + prompts.
// Private to the library: attention.hip declares these three and has checked every argument before it calls them.
#include "attn_walk.h"

bool lpi_attn_long_ok(int L, int causal, const void* row_start) { return !causal && !row_start && L > 288 && L <= 1024; }

int lpi_attn_long_fwd(int dtype, int B, int L, int H, const void* qkv, int ldqkv, void* ctx, int ldctx, float* lse, hipStream_t s) {
    return walk_fwd<64>(dtype, WalkArgs{B, L, H, qkv, ldqkv, ctx, ldctx, nullptr, 0, lse, nullptr, nullptr, 0}, s);
}

int lpi_attn_long_bwd(int dtype, int B, int L, int H, const void* qkv, int ldqkv, const void* ctx, int ldctx, const void* dctx, int lddctx, const float* lse,
                      float* delta, void* dqkv, int lddqkv, hipStream_t s) {
    return walk_bwd<64>(dtype, WalkArgs{B, L, H, qkv, ldqkv, ctx, ldctx, dctx, lddctx, const_cast<float*>(lse), delta, dqkv, lddqkv}, s);
}
