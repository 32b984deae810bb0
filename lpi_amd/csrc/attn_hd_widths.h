// Internal to the library: the host launches of the key-walking attention (attn_walk.h) at the head widths that live in translation units of their own —
// 88 (attn_hd88.hip) and 104 (attn_hd104.hip).  Plain C++ functions, no part of the C ABI: lpi_attn_hd_fwd / _bwd of attn_hd.hip stay the only entry points,
// check every argument and dispatch on head_dim.  The argument struct mirrors attn_walk.h's WalkArgs, which lives in each unit's anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>

struct AttnHdCall {
    int B, L, H;
    const void* qkv; int ldqkv;
    const void* ctx; int ldctx;
    const void* dctx; int lddctx;
    float* lse; float* delta;
    void* dqkv; int lddqkv;
};

// -> 0, LPI_EINVAL for an unknown dtype, or the launch's error (as walk_fwd / walk_bwd)
int attn_hd88_fwd(int dtype, const AttnHdCall& c, hipStream_t s);
int attn_hd88_bwd(int dtype, const AttnHdCall& c, hipStream_t s);
int attn_hd104_fwd(int dtype, const AttnHdCall& c, hipStream_t s);
int attn_hd104_bwd(int dtype, const AttnHdCall& c, hipStream_t s);
