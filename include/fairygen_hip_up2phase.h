/*
 * fairygen_hip_up2phase.h — an extension of the C ABI of libfairygen_hip.so (fairygen_hip.h, whose contract holds here unchanged:
 * stream-ordered, caller-owned buffers, no allocation, no host synchronisation, no atomics): the nearest-2x upsample + 3x3 Conv2d of
 * the VAE decoder's Resample38 as FOUR 2x2 convolutions over the low-resolution input, one per output phase.  It computes what
 * fg_conv3d_cl_bf16 computes with resample == 1, with 4 taps per output pixel in place of 9.  The main header, the other extension
 * headers and their versions stay as they are; a host that wants these entry points includes this header, checks
 * fg_conv_up2phase_version() and binds them next to the other tables.  tests/test_conv_up2_phase.py holds the
 * contract and the argument checks.
 *
 * THE IDENTITY.  Output pixel (2y + a, 2x + b), a, b in {0, 1}, of a 3x3 convolution (zero padding 1) over the nearest-2x upsampled
 * image reads, through its tap rows dy = 0, 1, 2, the upsampled rows 2y + a - 1 .. 2y + a + 1, which are only two low-resolution rows:
 * y - 1 (tap 0) and y (taps 1, 2) for a = 0; y (taps 0, 1) and y + 1 (tap 2) for a = 1; columns likewise.  So with
 *     R_0(0) = {0}, R_0(1) = {1, 2}, R_1(0) = {0, 1}, R_1(1) = {2}
 *     W_ab[i][j] = sum over dy in R_a(i), dx in R_b(j) of W[dy][dx]                                     (i, j in {0, 1})
 *     out(2y + a, 2x + b) = bias + sum over i, j of W_ab[i][j] . x(y + i - 1 + a, x + j - 1 + b)       (zero outside the image)
 * An upsampled padding row or column maps to a low-resolution row or column that is out of range, so the zero padding carries over.
 *
 * NUMERICS.  The summed weights are formed in fp32 and rounded ONCE to bf16 (round to nearest even); the products accumulate in fp32,
 * the bias is added in fp32 and the result rounded to bf16, as in fg_conv3d_cl_bf16.  The result is therefore NOT bit-identical to the
 * 9-tap form in general (bf16(W1 + W2) . x against W1 . x + W2 . x: a relative 2^-9 on a weight, the order of the bf16 storage of the
 * weights themselves); it IS bit-identical wherever every summed weight is a bf16 number and the fp32 sums are exact.
 */
#ifndef FAIRYGEN_HIP_UP2PHASE_H
#define FAIRYGEN_HIP_UP2PHASE_H

#include "fairygen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fg_conv_up2phase_version(void);      /* version of this extension, currently 1 */

/* Bytes of the phase-packed weights of a (Cout, Cin, 1, 3, 3) convolution: 16 tap matrices [phase 2a + b][tap 2i + j][Cout padded to
 * 128][Cin] bf16; 0 for arguments fg_conv_up2phase_pack_bf16 refuses. */
int64_t fg_conv_up2phase_packed_bytes(int Cout, int Cin);

/* w (Cout, Cin, 1, 3, 3) bf16, contiguous (= (Cout, Cin, 3, 3)) -> packed (fg_conv_up2phase_packed_bytes): the 16 matrices W_ab[i][j]
 * above, each laid out as fg_conv_pack_weight_bf16 lays out a tap ([cout][cin], cin contiguous, rows past Cout zero).  Needs
 * Cin % 64 == 0.  Run once per checkpoint. */
int fg_conv_up2phase_pack_bf16(const void* w, void* packed, int Cout, int Cin, fg_stream_t stream);

/* x (T, H/2, W/2, Cin) channels-last -> out (T, H, W, Cout) = fg_conv3d_cl_bf16(resample = 1, no residual, no time interleave) in the
 * phase form.  T, H, W, Cin, Cout, kt, ks as there (H, W the OUTPUT size).  Refused: odd H or W, kt != 1, ks != 3, Cin % 64 != 0,
 * Cout % 4 != 0, an input or output of 3.5 GiB or more (32-bit offsets).  x and w_phase 16-byte aligned, bias and out 8-byte. */
int fg_conv3d_up2_phase_bf16(const void* x, const void* w_phase, const void* bias, void* out, int T, int H, int W, int Cin, int Cout,
                             int kt, int ks, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRYGEN_HIP_UP2PHASE_H */
