// postprocess_value.h -- the value of Sam.postprocess_masks (modeling/sam.py:133-162) at an output pixel, from the 256^2 logits.
// ONE definition for every kernel that needs it: postprocess_kernel (decoder_kernels.hip) thresholds / stores these values,
// score_masks_kernel (quality_kernels.hip) counts them against thresholds, and the count at threshold 0 must equal the set bytes of
// the mask exactly.
//
// Why a macro and not an inline function: HIP compiles with -ffp-contract=fast, and which product of `a * b + c * d` ends up inside
// the FMA (and whether a packed multiply + add is used instead) is decided late, after vectorisation, from the code around the
// expression.  Moving these statements into a __forceinline__ function changed postprocess_kernel's instructions (3 multiply-add
// pairs became FMAs: other roundings, so other logits in the last place).  Expanded as text, postprocess_kernel compiles to the
// instructions it had before the statements moved here (checked on the assembly), so its output bytes are unchanged.
// Nothing but the compiler making the same choices twice ties score_masks_kernel to it: tests/test_quality_gpu.py asks for exact
// equality of the counts with the mask bytes on every route, and is what would notice a compiler that chooses differently.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

// PyTorch upsample_bilinear2d, align_corners=False: src = scale*(dst+0.5)-0.5 clamped at 0,
// scale = in/out; out = wy0*(wx0*v00 + wx1*v01) + wy1*(wx0*v10 + wx1*v11).
struct Lin {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ Lin lin_coord(int dst, float scale, int in_size) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Lin r;
    r.i0 = (int)src;
    r.i0 = r.i0 < in_size - 1 ? r.i0 : in_size - 1;
    r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
    r.w1 = src - (float)r.i0;
    r.w0 = 1.0f - r.w1;
    return r;
}
// stage 1: value of the img_size^2 upsampled map at integer (Y1, X1), from the 256^2 logits
__device__ __forceinline__ float stage1(const float* __restrict__ low, int LS, float s1, int Y1, int X1) {
    const Lin ly = lin_coord(Y1, s1, LS), lx = lin_coord(X1, s1, LS);
    const float* r0 = low + (size_t)ly.i0 * LS;
    const float* r1 = low + (size_t)ly.i1 * LS;
    return ly.w0 * (lx.w0 * r0[lx.i0] + lx.w1 * r0[lx.i1]) + ly.w1 * (lx.w0 * r1[lx.i0] + lx.w1 * r1[lx.i1]);
}

// Expands, in a kernel, to the statements that compute `float v[4]`: v[e] = the postprocessed logit at output pixel (Y, X0 + e) of
// the H x W output for an in_h x in_w input frame, 0 for the pixels past W.  Reads the names low (one mask's LS x LS logits, LS =
// img_size / 4), LS, in_h, in_w, H, W, img_size, Y, X0 (X0 % 4 == 0) from the enclosing scope; declares s1, identity and v.
#define SAMRS_POSTPROCESS_VALUES()                                                                                                              \
    const float s1 = (float)LS / (float)img_size;                                                                                               \
    const bool identity = (H == in_h) && (W == in_w);                                                                                           \
    float v[4];                                                                                                                                 \
    if (identity && 4 * LS == img_size && X0 + 3 < W) {                                                                                         \
        /* the case of every 1024^2 tile: scale exactly 1/4, so output columns 4k, 4k+1 interpolate between the same two */                     \
        /* logits columns, and 4k+2, 4k+3 between the next pair; one row pair serves all four.  Same expression per */                          \
        /* pixel as stage1 (bit-identical), 8 loads and 5 coordinate computations instead of 16 and 8. */                                       \
        const Lin ly = lin_coord(Y, s1, LS);                                                                                                    \
        const float* r0 = low + (size_t)ly.i0 * LS;                                                                                             \
        const float* r1 = low + (size_t)ly.i1 * LS;                                                                                             \
        const Lin la = lin_coord(X0, s1, LS), lb = lin_coord(X0 + 1, s1, LS), lc = lin_coord(X0 + 2, s1, LS), ld = lin_coord(X0 + 3, s1, LS);   \
        const float a00 = r0[la.i0], a01 = r0[la.i1], a10 = r1[la.i0], a11 = r1[la.i1];                                                         \
        const float c00 = r0[lc.i0], c01 = r0[lc.i1], c10 = r1[lc.i0], c11 = r1[lc.i1];                                                         \
        v[0] = ly.w0 * (la.w0 * a00 + la.w1 * a01) + ly.w1 * (la.w0 * a10 + la.w1 * a11);                                                       \
        v[1] = ly.w0 * (lb.w0 * a00 + lb.w1 * a01) + ly.w1 * (lb.w0 * a10 + lb.w1 * a11);                                                       \
        v[2] = ly.w0 * (lc.w0 * c00 + lc.w1 * c01) + ly.w1 * (lc.w0 * c10 + lc.w1 * c11);                                                       \
        v[3] = ly.w0 * (ld.w0 * c00 + ld.w1 * c01) + ly.w1 * (ld.w0 * c10 + ld.w1 * c11);                                                       \
    } else if (identity) {                                                                                                                      \
    _Pragma("unroll")                                                                                                                              \
        for (int e = 0; e < 4; ++e) v[e] = (X0 + e < W) ? stage1(low, LS, s1, Y, X0 + e) : 0.f;                                                 \
    } else {                                                                                                                                    \
        const float sy = (float)in_h / (float)H, sx = (float)in_w / (float)W;                                                                   \
        const Lin ly = lin_coord(Y, sy, in_h);                                                                                                  \
    _Pragma("unroll")                                                                                                                              \
        for (int e = 0; e < 4; ++e) {                                                                                                           \
            if (X0 + e < W) {                                                                                                                   \
                const Lin lx = lin_coord(X0 + e, sx, in_w);                                                                                     \
                const float a = lx.w0 * stage1(low, LS, s1, ly.i0, lx.i0) + lx.w1 * stage1(low, LS, s1, ly.i0, lx.i1);                          \
                const float b = lx.w0 * stage1(low, LS, s1, ly.i1, lx.i0) + lx.w1 * stage1(low, LS, s1, ly.i1, lx.i1);                          \
                v[e] = ly.w0 * a + ly.w1 * b;                                                                                                   \
            } else {                                                                                                                            \
                v[e] = 0.f;                                                                                                                     \
            }                                                                                                                                   \
        }                                                                                                                                       \
    }
