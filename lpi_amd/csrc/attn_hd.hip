// Multi-head attention for heads that are NOT 64 wide (non-causal, uniform sequences, 1 <= L <= 1024): the key-walking family of attn_walk.h at HD = 80, the one
// such width that ships — OpenCLIP ViT-H/14's vision tower (width 1280 = 16 heads of 80; 257 tokens + prompts).
//
// replaces: nn.MultiheadAttention of a vision tower whose width / heads != 64 (retrieval/models/clip/model.py:183-185 computes width // 64 heads and cannot
// build such a tower; open_clip's ViT-H-14 has head_width 80).
#include "attn_walk.h"

namespace {

constexpr int HDW = 80;      // the one head width that ships

inline bool hd_shape_ok(int L, int H, int head_dim) { return head_dim == HDW && L > 0 && L <= 1024 && H > 0; }
// B H is the grid's y extent
inline bool hd_bad(int dtype, int B, int L, int H, int head_dim) {
    return (dtype != LPI_F32 && dtype != LPI_BF16 && dtype != LPI_F16) || !hd_shape_ok(L, H, head_dim) || B <= 0 || (long long)B * H > 65535;
}
inline bool hd_bad_ld(int ld, int cols, int esz) { return ld < cols || ((long long)ld * esz) % 16 != 0; }

}  // namespace

extern "C" int lpi_attn_hd_supported(int L, int H, int head_dim) { return hd_shape_ok(L, H, head_dim) ? 1 : 0; }

extern "C" int lpi_attn_hd_fwd(int dtype, int B, int L, int H, int head_dim, const void* qkv, int ldqkv, void* ctx, int ldctx, float* lse, void* stream) {
    if (hd_bad(dtype, B, L, H, head_dim) || !qkv || !ctx || !lse) return LPI_EINVAL;
    const int esz = dtype == LPI_F32 ? 4 : 2;
    if (hd_bad_ld(ldqkv, 3 * H * HDW, esz) || ldctx < H * HDW || (ldctx & 7)) return LPI_EINVAL;
    if (((uintptr_t)qkv | (uintptr_t)ctx) & 15) return LPI_EINVAL;
    return walk_fwd<HDW>(dtype, WalkArgs{B, L, H, qkv, ldqkv, ctx, ldctx, nullptr, 0, lse, nullptr, nullptr, 0}, (hipStream_t)stream);
}

extern "C" int lpi_attn_hd_bwd(int dtype, int B, int L, int H, int head_dim, const void* qkv, int ldqkv, const void* ctx, int ldctx, const void* dctx, int lddctx,
                               const float* lse, float* delta, void* dqkv, int lddqkv, void* stream) {
    if (hd_bad(dtype, B, L, H, head_dim) || !qkv || !ctx || !dctx || !lse || !delta || !dqkv) return LPI_EINVAL;
    const int esz = dtype == LPI_F32 ? 4 : 2;
    if (hd_bad_ld(ldqkv, 3 * H * HDW, esz) || hd_bad_ld(lddqkv, 3 * H * HDW, esz) || hd_bad_ld(ldctx, H * HDW, esz) || hd_bad_ld(lddctx, H * HDW, esz)) return LPI_EINVAL;
    if (((uintptr_t)qkv | (uintptr_t)ctx | (uintptr_t)dctx | (uintptr_t)dqkv) & 15) return LPI_EINVAL;
    return walk_bwd<HDW>(dtype, WalkArgs{B, L, H, qkv, ldqkv, ctx, ldctx, dctx, lddctx, const_cast<float*>(lse), delta, dqkv, lddqkv}, (hipStream_t)stream);
}
