// fp32-accurate Conv1d on the 16-bit matrix pipe ("split precision"): every fp32 operand, scaled by a power of two, is split into
// TWO fp16 planes (a s = h0 + h1, 22 significant bits; both differences exact in fp32) and the three significant cross products
// h0 h0', h0 h1', h1 h0' are accumulated in fp32 by v_mfma_f32_32x32x16_f16 (the dropped h1 h1' term is < 2^-22 relative).
// Measured against an fp64 reference the result carries the error of an fp32 GEMM - rel. 4.5e-7 at K = 768, below a 3 x bf16 / 6
// product split (6.8e-7: twice the accumulations) and below numpy's sgemm (7.0e-7) - tools/ubench/gemm_x3v.hip - at 3 matrix
// instructions per 16 channels instead of 8 v_mfma_f32_32x32x2_f32 (96 SIMD-cycles against 512).
//
// Operand layout in HBM - 16-byte chunks = 8 consecutive channels of one plane:
//   w3 [tap][Cin/8][2][CoutP][8 fp16]    split once at bind time from the fp32 packed weights  (launch_split_weights), x XS_SCALE_W
//   x3 [b][Cin/8][2][Tp][8 fp16]         written by the producer side (launch_split_planes / launch_gn_split_planes: GroupNorm affine
//                                        + SiLU + zero padding + per-sample length folded in), x XS_SCALE_X; Tp = round_up(T, 192) + 2
//                                        halo columns
// A K-step (16 channels) of a tile is 4 contiguous runs (plane, k-half) in HBM and in LDS, so both tiles are moved by LDS-DMA and every
// ds_read_b128 of an MFMA fragment is bank-conflict-free with no padding or swizzle.
#pragma once
#include "conv_gemm.h"

namespace dtts {

constexpr int X3_HALO = 1;   // zero columns on each side of the time axis (covers k = 3, dilation 1)
constexpr int X3_BN = 192;   // N tile of the conv kernel: 936 mel frames = 4.875 tiles (2.5 % padding; 128 would pad 8.6 %)
static inline int x3_tp(int T) { return round_up(T, X3_BN) + 2 * X3_HALO; }
static inline size_t x3_bytes(int B, int C, int T) { return (size_t)B * (C / 8) * 2 * x3_tp(T) * 16; }

// wp: fp32 packed weights [KW][CinP][CoutP] -> out [KW][CinP/8][2][CoutP][8 fp16]
void launch_split_weights(const float* wp, int KW, int CinP, int CoutP, void* out, hipStream_t s);
// x [B][C][T] fp32 (strides) -> x3; v = act(a*x + d) with (a, d) = ab[b][c][0..1] (ab may be null); zero outside [0, len[b])
void launch_split_planes(const float* x, long long x_bs, int x_cs, const float* ab, int act, const int* lens, int T, int B, int C,
                         void* out, hipStream_t s);
// the KW-tap expansion of x as planes [B][KW * C/8][2][x3_tp(T)][8 fp16] (chunk (tap, c8), column t = x[c][t + tap - pad], zero outside
// [0, len)): a k = KW conv with "same" padding becomes a 1x1 conv_x3 launch over KW * C input channels on the SAME w3 image - the route
// the flow's WaveNet in_layers (k = 5, gated) take onto conv_x3's small-launch pipeline.  sat as launch_split_planes_ex.
void launch_split_planes_taps(const float* x, long long x_bs, int x_cs, const int* lens, int T, int B, int C, int KW, int pad, void* out,
                              hipStream_t s, int* sat = nullptr);
// GroupNorm (statistics + affine, optional AdaGN (1 + scale, shift) from `ada`) + activation + split in one pass; arguments as
// launch_gn_coeffs (ops.h), x_bmod included
void launch_gn_split_planes(const float* x, long long x_bs, int x_cs, const int* lens, int T, int B, int C, int groups,
                            const float* gamma, const float* beta, float eps, const float* ada, int ada_stride, int ada_bs, int act,
                            void* out, hipStream_t s, const int* ada_idx = nullptr, int x_bmod = 0);
// uses p.w3 / p.x3 / p.x3_tp (+ the epilogue fields of ConvParams); stride 1, dilation 1, pad <= X3_HALO, no phases; gate (tanh * sigmoid on packed row pairs) + badd only
// as a 1x1 conv without residual (EPI 4: the WaveNet in_layers over launch_split_planes_taps planes)
// p.p1 (the trunk's fp16 mode, option "trunk_fp16"): ONE product h0 h0' on plane 0 of the same images, 32 channels per K-step, instead of
// three (Cin a multiple of 32, no gate); plane 1 is neither fetched nor multiplied (conv_x3.hip)
// `chosen` (host side, may be null): what the launcher picked for this launch, filled just before the launch - the instantiation
// (epi 0, 1, 2 or 4, kw3, stages 2..4, p1), the split, the epilogue form (epi_vec 1: LDS-staged 16-byte stores, 0: scalar), whether a live-column
// table is attached and the grid size.  How tests/test_gpu_conv_x3.py asserts that a case ran the variant it was written for.
struct ConvX3Launch {
    int epi = -1, kw3 = 0, stages = 0, ksplit = 0, p1 = 0, epi_vec = 0, cols = 0, workgroups = 0;
};
void launch_conv_x3(const ConvParams& p, hipStream_t s, ConvX3Launch* chosen = nullptr);
// the launcher's split-K rule (host): the workgroups per output tile of a launch of B samples x Nout columns (1: no split), decided on
// the padded tile count; ksplit_max > 0 caps it.  For callers that must know before launching whether a launch's width picks its
// summation order (Model::integ_unsplit).
int conv_x3_ksplit(int CoutP, int Cin, int KW, int Nout, int B, int ksplit_max = 0);
// option "conv_stages" (process-wide): 2 / 3 / 4 forces that many LDS stages, 0 = by launch size (the launcher's rule), n < 0 = back to
// the initial value (DTTS_CONV_STAGES, else 0)
void set_conv_stages(int n);

// Split scratch of a launch stream (conv_x3's split-K slabs; the trunk attention's key-split partials use the same slot: launches on one
// stream are ordered): `part` = nslabs slabs of X3_SLAB_FLOATS floats, `count` = X3_SPLIT_COUNTERS arrival counters that are zero
// between launches (the reducing workgroup / wave resets its counter).
constexpr size_t X3_SLAB_FLOATS = 96 * 256, X3_MAX_SLABS = 1024, X3_SPLIT_COUNTERS = 4096;
void x3_split_workspace(hipStream_t s, size_t nslabs, float** part, int** count);

// ---- dilated / wide-kernel variant (conv_x3d.hip): HiFiGAN ResBlock1 convs, k = 3 / 7 / 11, any dilation with (k - 1) dil <= 64
constexpr int X3D_HALO = 32;                          // left zero columns of its planes (>= the largest pad: (11 * 5 - 5) / 2 = 25)
static inline int x3d_tp(int T) { return round_up(T, X3_BN) + 64 + X3D_HALO; }
static inline size_t x3d_bytes(int B, int CP, int T) { return (size_t)B * (CP / 8) * 2 * x3d_tp(T) * 16; }
// x [B][C][T] fp32 -> planes [B][CP/8][2][Tp][8 fp16], `halo` zero columns on the left, zero chunks for channels C .. CP - 1
// sat (may be null): device flag set to 1 when a scaled value lies beyond fp16's range (the planes saturate there)
void launch_split_planes_ex(const float* x, long long x_bs, int x_cs, int act, float slope, const int* lens, int T, int B, int C, int CP,
                            int halo, int Tp, void* out, hipStream_t s, int* sat = nullptr);
// p.w3 / p.x3 / p.x3_tp / p.x3_halo, p.Cin = padded input channels; stride 1, no gate / phases / badd.  p.next3: act(y) written also
// (p.y == null: only) as the planes of the NEXT conv - live columns; the buffer's margins are zeroed by launch_zero_plane_margins
void launch_conv_x3d(const ConvParams& p, hipStream_t s);
void launch_zero_plane_margins(const int* lens, int T, int B, int CP, int halo, int Tp, void* out, hipStream_t s);

}  // namespace dtts
