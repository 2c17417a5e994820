// Stride-2 convolution at fp32 accuracy on the gfx950 BF16 matrix cores: forward, input gradient and weight gradient of
// nn.Conv2d(k = 3, stride = 2, padding = 1), dense and grouped (one launch per pass), plus the two memory-bound helpers of the
// 1x1 / 2 shortcuts (2x2 sub-sampling and its adjoint).
//
// Geometry: input H x W, output Ho x Wo = ceil(H/2) x ceil(W/2); output pixel (yo, xo) is centred on input pixel (2yo, 2xo).
// Arithmetic: the split-bf16 scheme of conv_split.hip / wgrad_split.hip (three exact bf16 terms per operand, six cross products,
// smallest first, fp32 accumulation).  No atomics; the order of accumulation depends on the channel counts only.
//
// Forward (conv_s2_fwd_kernel): the implicit GEMM of conv_split.hip -- M = 32 output pixels of a row, N = 32 output channels,
// K = 8 input channels x 2 taps -- on the UNCHANGED stride-1 packed filter.  The (2 TY + 1)-row input tile is staged into LDS
// de-interleaved by column parity (per row an even-column and an odd-column run of 16-byte slots), so the A fragment of tap kx is
// 32 consecutive slots of one parity run: the ds_read_b128 keeps the 16-byte lane stride of the stride-1 kernel.
//
// Input gradient (conv_s2_dgrad_kernel): on the UNCHANGED transposed packed filter of the stride-1 input gradient, with no
// zero-stuffed intermediate.  An M tile is 32 dx pixels of one row and one column parity; of the 9 taps of the flipped filter a
// parity class (py, px) meets only those that land on a sample of dy (1, 2, 2, 4 taps).  The packed filter pairs consecutive taps
// in one K step, so a lane half whose tap is dead for the class reads an all-zero LDS slot and a step with two dead taps is
// skipped: 1 + 2 + 2 + 4 = 9 K steps per 8 channels and 2 x 2 pixels where the zero-stuffed stride-1 pass issues 20 (a per-class
// filter layout would need 4.5).  A lane interleaves its px = 0 / px = 1 results in registers: dx is written with 16-byte
// stores, every element exactly once (zeros where no tap reaches).
//
// Weight gradient (conv_s2_wgrad_kernel): per tap a GEMM M = 16 output channels, N = 16 input channels, K = 32 output pixels of a
// row on v_mfma_f32_16x16x32_bf16.  The x tile is staged pixel-contiguous in THREE planes per row -- columns 2xo - 1, 2xo and
// 2xo + 1 -- so the operand of tap kx is an aligned 16-byte read of plane kx.  A block owns 64 x 16 channels (a wave: 16 x 16,
// nine accumulator tiles), walks image tiles grid-stride and stores its partial sums once into its own workspace slice in the
// packed [split][co 16][ci 16][tap][16][16] layout of wgrad_split.hip; conv_wgrad.hip's unpack adds the slices in a fixed order.
#include "cd_common.h"
#include "conv_split.h"
#include "conv_strided.h"
#include "split_bf16.h"

namespace cd {

// The filters are the stride-1 split packs of a 3x3 convolution, whose geometry conv_split.h owns (split_dy, split_steps,
// split_ntiles, SPLIT_STEP_UNITS): with <= 16 output channels a column tile holds 16 channels x 2 output rows (taps over 4 filter
// rows), of which only columns 0..15 -- the unshifted filter -- are used here.

// One forward / input-gradient launch.  src: the tensor the reduction runs over (x, or dy), dst: the result (y, or dx);
// H x W: the un-strided extents (x / dx), Ho x Wo the strided ones (y / dy).
struct S2Args {
    const float* src; const u32x4* wsp; const float* bias; float* dst;
    int s_ctot, s_coff, IC, d_ctot, d_coff, OC, accumulate, H, W, Ho, Wo, tiles_x, tiles_y, g_s, g_d;
    size_t g_w;
};

// ---------------------------------------------------------------- forward
constexpr int S2F_TY = 8, S2F_ROWS = 2 * S2F_TY + 1, S2F_PW = 36, S2F_RS = 2 * S2F_PW, S2F_PLANE = S2F_ROWS * S2F_RS;
constexpr size_t S2F_LDS = (size_t)3 * S2F_PLANE * 16;

template <int DYL>
__global__ __launch_bounds__(kBlock, 2) void conv_s2_fwd_kernel(const S2Args a) {
    constexpr int TY = S2F_TY, ROWS = S2F_ROWS, PW = S2F_PW, RS = S2F_RS, PLANE = S2F_PLANE, KSTEPS = split_steps(3, DYL);
    constexpr int QUADS = RS / 4, UNITS = ROWS * QUADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char s2_smem[];
    u32x4* s_in = reinterpret_cast<u32x4*>(s2_smem);   // [3 splits][ROWS][parity][PW] 16-byte slots (8 bf16 channels of one pixel)

    const int grp = (int)blockIdx.z, ct = (int)blockIdx.y;
    int t_lin = (int)blockIdx.x;
    const int tiles_img = a.tiles_x * a.tiles_y;
    const int n = t_lin / tiles_img; t_lin -= n * tiles_img;
    const int ty = t_lin / a.tiles_x, tx = t_lin - ty * a.tiles_x;
    const int X0 = tx * 32, Y0 = ty * TY;                  // output coordinates
    const int H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo, IC = a.IC, OC = a.OC;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, li = lane & 31, g = lane >> 5;
    const size_t HW = (size_t)H * W;
    const float* xin = a.src + ((size_t)n * a.s_ctot + a.s_coff + grp * a.g_s) * HW;
    const int n_chunks = (IC + 7) / 8;
    const bool vec_in = (W & 3) == 0;
    const u32x4* wt = a.wsp + (size_t)grp * a.g_w + (size_t)ct * n_chunks * KSTEPS * SPLIT_STEP_UNITS + lane;

    f32x16 acc[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[m][q] = 0.f;

    // LDS slot (without the M-tile's row and the lane's pixel) of this lane half's tap in every K step
    int tap_slot[KSTEPS];
#pragma unroll
    for (int st = 0; st < KSTEPS; ++st) {
        const int tap = 2 * st + g, kyp = tap / 3, kx = tap - 3 * kyp;
        // input column 2 (X0 + i) + kx - 1 = tile column 2 i + kx + 3: kx = 0 -> odd run, slot i + 1; 1 -> even run, i + 2; 2 -> odd run, i + 2
        tap_slot[st] = kyp < 3 ? kyp * RS + ((kx & 1) ? 0 : PW) + (kx == 0 ? 1 : 2) : 0;   // (a padded tap carries zero weights: any valid slot)
    }

    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        // the chunk's weight fragments: in flight during the staging
        bf16x8 b[KSTEPS][3];
#pragma unroll
        for (int st = 0; st < KSTEPS; ++st)
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) b[st][sp] = __builtin_bit_cast(bf16x8, wt[((size_t)chunk * KSTEPS + st) * SPLIT_STEP_UNITS + sp * 64]);
        __syncthreads();   // the previous chunk's tile is consumed
        for (int u = threadIdx.x; u < UNITS; u += kBlock) {
            const int r = u / QUADS, q4 = (u - r * QUADS) * 4;
            const int gy = 2 * Y0 - 1 + r, gx = 2 * X0 - 4 + q4;
            const bool row_in = (unsigned)gy < (unsigned)H;
            const float* rowp = xin + (size_t)(row_in ? gy : 0) * W;
            float v[8][4];
            unsigned keep[4];
            if (vec_in) {       // W % 4 == 0: an aligned quad is inside or outside the image as a whole
                const bool in = row_in && (unsigned)gx < (unsigned)W;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int ci = chunk * 8 + c;
                    const float4 f = *reinterpret_cast<const float4*>(rowp + (in ? gx : 0) + (size_t)(ci < IC ? ci : IC - 1) * HW);
                    v[c][0] = f.x; v[c][1] = f.y; v[c][2] = f.z; v[c][3] = f.w;
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) keep[p] = in ? 0xffffffffu : 0u;
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const bool in = row_in && (unsigned)(gx + p) < (unsigned)W;
                    keep[p] = in ? 0xffffffffu : 0u;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const int ci = chunk * 8 + c;
                        v[c][p] = rowp[(in ? gx + p : 0) + (size_t)(ci < IC ? ci : IC - 1) * HW];
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                u32x4 hh, mm, ll;
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2) {
                    const unsigned k0 = keep[p] & (chunk * 8 + 2 * c2 < IC ? 0xffffffffu : 0u), k1 = keep[p] & (chunk * 8 + 2 * c2 + 1 < IC ? 0xffffffffu : 0u);
                    unsigned h, m, l;   // zero padding (pixels and channels) stays an exact zero
                    split_pair(__uint_as_float(__float_as_uint(v[2 * c2][p]) & k0), __uint_as_float(__float_as_uint(v[2 * c2 + 1][p]) & k1), h, m, l);
                    hh[c2] = h; mm[c2] = m; ll[c2] = l;
                }
                const int c = q4 + p, slot = r * RS + (c & 1) * PW + (c >> 1);
                s_in[slot] = hh; s_in[PLANE + slot] = mm; s_in[2 * PLANE + slot] = ll;
            }
        }
        __syncthreads();
#pragma unroll
        for (int st = 0; st < KSTEPS; ++st) {
            bf16x8 av[2][3];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int slot = tap_slot[st] + 2 * (wid + 4 * m) * RS + li;
                av[m][0] = __builtin_bit_cast(bf16x8, s_in[slot]);
                av[m][1] = __builtin_bit_cast(bf16x8, s_in[PLANE + slot]);
                av[m][2] = __builtin_bit_cast(bf16x8, s_in[2 * PLANE + slot]);
            }
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int m = 0; m < 2; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[m][SPLIT_PA[p]], b[st][SPLIT_PB[p]], acc[m], 0, 0, 0);
        }
    }

    // ---- epilogue.  D: lane holds column lane & 31, pixels 8q + 4g + {0..3}
    const int co = DYL == 2 ? li : ct * 32 + li;
    if ((DYL == 2 && li >= 16) || co >= OC) return;
    const int ch = a.d_coff + grp * a.g_d + co;
    const float bv = a.bias != nullptr ? a.bias[grp * a.g_d + co] : 0.f;
    float* yout = a.dst + ((size_t)n * a.d_ctot + ch) * Ho * Wo;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int gy = Y0 + wid + 4 * m;
        if (gy >= Ho) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gx = X0 + 8 * q + 4 * g;
            float e[4] = {acc[m][4 * q] + bv, acc[m][4 * q + 1] + bv, acc[m][4 * q + 2] + bv, acc[m][4 * q + 3] + bv};
            float* d = yout + (size_t)gy * Wo + gx;
            if ((Wo & 3) == 0 && gx < Wo) {
                if (a.accumulate) {
                    const float4 o = *reinterpret_cast<const float4*>(d);
                    e[0] += o.x; e[1] += o.y; e[2] += o.z; e[3] += o.w;
                }
                *reinterpret_cast<float4*>(d) = make_float4(e[0], e[1], e[2], e[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (gx + k < Wo) d[k] = a.accumulate ? d[k] + e[k] : e[k];
            }
        }
    }
}

// ---------------------------------------------------------------- input gradient
constexpr int S2D_TA = 4, S2D_ROWS = S2D_TA + 1, S2D_RS = 36, S2D_PLANE = S2D_ROWS * S2D_RS, S2D_CG = 4;
constexpr int S2D_ZERO = S2D_CG * 3 * S2D_PLANE;     // the all-zero slot behind the images
constexpr size_t S2D_LDS = (size_t)(S2D_ZERO + 1) * 16;

// tap t = ky' * 3 + kx' of the flipped filter meets a sample of dy for the dx parity class (py, px)
__host__ __device__ constexpr bool s2d_live(int t, int py, int px) { return t < 9 && ((py + t / 3 + 1) & 1) == 0 && ((px + t % 3 + 1) & 1) == 0; }
// its dy pixel relative to (row a, column b) of dx pixel (2a + py, 2b + px)
__host__ __device__ constexpr int s2d_off(int t, int py, int px) { return ((py + t / 3 - 1) / 2) * S2D_RS + (px + t % 3 - 1) / 2; }

template <int DYL>
__global__ __launch_bounds__(kBlock, 2) void conv_s2_dgrad_kernel(const S2Args a) {
    constexpr int TA = S2D_TA, ROWS = S2D_ROWS, RS = S2D_RS, PLANE = S2D_PLANE, CG = S2D_CG, KSTEPS = split_steps(3, DYL), LIVE_STEPS = 5;
    constexpr int QUADS = RS / 4, UNITS = ROWS * QUADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char s2_smem[];
    u32x4* s_in = reinterpret_cast<u32x4*>(s2_smem);   // [CG chunks][3 splits][ROWS][RS] slots + the zero slot

    const int grp = (int)blockIdx.z, ct = (int)blockIdx.y;
    int t_lin = (int)blockIdx.x;
    const int tiles_img = a.tiles_x * a.tiles_y;
    const int n = t_lin / tiles_img; t_lin -= n * tiles_img;
    const int ty = t_lin / a.tiles_x, tx = t_lin - ty * a.tiles_x;
    const int X0 = tx * 32, A0 = ty * TA;                  // dy coordinates; dx rows 2 A0 .., columns 2 X0 ..
    const int H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo, IC = a.IC, OC = a.OC;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, li = lane & 31, g = lane >> 5;
    const size_t HWo = (size_t)Ho * Wo;
    const float* din = a.src + ((size_t)n * a.s_ctot + a.s_coff + grp * a.g_s) * HWo;
    const int n_chunks = (IC + 7) / 8;
    const bool vec_in = (Wo & 3) == 0;
    const u32x4* wt = a.wsp + (size_t)grp * a.g_w + (size_t)ct * n_chunks * KSTEPS * SPLIT_STEP_UNITS + lane;
    if (threadIdx.x == 0) s_in[S2D_ZERO] = u32x4{0u, 0u, 0u, 0u};   // (visible after the first barrier)

    f32x16 acc[2][2];   // [py][px] of this wave's dx row pair 2 (A0 + wid) + py
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    const int abase = wid * RS + li;
    for (int round = 0; round * CG < n_chunks; ++round) {
        __syncthreads();   // the previous round's images are consumed
        for (int uu = threadIdx.x; uu < CG * UNITS; uu += kBlock) {
            const int cg = uu / UNITS, u = uu - cg * UNITS, chunk = round * CG + cg;
            if (chunk >= n_chunks) break;
            const int r = u / QUADS, q4 = (u - r * QUADS) * 4;
            const int gy = A0 + r, gx = X0 + q4;
            const bool row_in = gy < Ho;
            const float* rowp = din + (size_t)(row_in ? gy : 0) * Wo;
            float v[8][4];
            unsigned keep[4];
            if (vec_in) {
                const bool in = row_in && gx < Wo;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int ci = chunk * 8 + c;
                    const float4 f = *reinterpret_cast<const float4*>(rowp + (in ? gx : 0) + (size_t)(ci < IC ? ci : IC - 1) * HWo);
                    v[c][0] = f.x; v[c][1] = f.y; v[c][2] = f.z; v[c][3] = f.w;
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) keep[p] = in ? 0xffffffffu : 0u;
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const bool in = row_in && gx + p < Wo;
                    keep[p] = in ? 0xffffffffu : 0u;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const int ci = chunk * 8 + c;
                        v[c][p] = rowp[(in ? gx + p : 0) + (size_t)(ci < IC ? ci : IC - 1) * HWo];
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                u32x4 hh, mm, ll;
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2) {
                    const unsigned k0 = keep[p] & (chunk * 8 + 2 * c2 < IC ? 0xffffffffu : 0u), k1 = keep[p] & (chunk * 8 + 2 * c2 + 1 < IC ? 0xffffffffu : 0u);
                    unsigned h, m, l;
                    split_pair(__uint_as_float(__float_as_uint(v[2 * c2][p]) & k0), __uint_as_float(__float_as_uint(v[2 * c2 + 1][p]) & k1), h, m, l);
                    hh[c2] = h; mm[c2] = m; ll[c2] = l;
                }
                const int slot = cg * 3 * PLANE + r * RS + q4 + p;
                s_in[slot] = hh; s_in[PLANE + slot] = mm; s_in[2 * PLANE + slot] = ll;
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int cg = 0; cg < CG; ++cg) {
            const int chunk = round * CG + cg;
            if (chunk >= n_chunks) break;   // block-uniform
            bf16x8 b[LIVE_STEPS][3];        // (the 4-row layout's sixth step holds filter row 3 only: dead for every class)
#pragma unroll
            for (int st = 0; st < LIVE_STEPS; ++st)
#pragma unroll
                for (int sp = 0; sp < 3; ++sp) b[st][sp] = __builtin_bit_cast(bf16x8, wt[((size_t)chunk * KSTEPS + st) * SPLIT_STEP_UNITS + sp * 64]);
            const int img = cg * 3 * PLANE + abase;
#pragma unroll
            for (int st = 0; st < LIVE_STEPS; ++st)
#pragma unroll
                for (int py = 0; py < 2; ++py)
#pragma unroll
                    for (int px = 0; px < 2; ++px) {
                        const bool l0 = s2d_live(2 * st, py, px), l1 = s2d_live(2 * st + 1, py, px);
                        if (!(l0 || l1)) continue;     // (compile-time after unrolling)
                        const int o0 = l0 ? s2d_off(2 * st, py, px) : 0, o1 = l1 ? s2d_off(2 * st + 1, py, px) : 0;
                        const bool lv = g ? l1 : l0;
                        const int slot = img + (g ? o1 : o0);
                        bf16x8 av[3];
#pragma unroll
                        for (int sp = 0; sp < 3; ++sp) av[sp] = __builtin_bit_cast(bf16x8, s_in[lv ? slot + sp * PLANE : S2D_ZERO]);
#pragma unroll
                        for (int p = 0; p < 6; ++p)
                            acc[py][px] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[SPLIT_PA[p]], b[st][SPLIT_PB[p]], acc[py][px], 0, 0, 0);
                    }
        }
    }

    // ---- epilogue: the lane's pixels 8q + 4g + {0..3} of px = 0 and px = 1 are the 8 consecutive dx columns 2 (X0 + 8q + 4g) ..
    const int co = DYL == 2 ? li : ct * 32 + li;
    if ((DYL == 2 && li >= 16) || co >= OC) return;
    float* dout = a.dst + ((size_t)n * a.d_ctot + a.d_coff + grp * a.g_d + co) * H * W;
#pragma unroll
    for (int py = 0; py < 2; ++py) {
        const int gy = 2 * (A0 + wid) + py;
        if (gy >= H) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gx = 2 * (X0 + 8 * q + 4 * g);
            float e[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) { e[2 * k] = acc[py][0][4 * q + k]; e[2 * k + 1] = acc[py][1][4 * q + k]; }
            float* d = dout + (size_t)gy * W + gx;
            if ((W & 3) == 0) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    if (gx + 4 * h < W) {
                        float4 o = make_float4(e[4 * h], e[4 * h + 1], e[4 * h + 2], e[4 * h + 3]);
                        if (a.accumulate) {
                            const float4 p4 = *reinterpret_cast<const float4*>(d + 4 * h);
                            o.x += p4.x; o.y += p4.y; o.z += p4.z; o.w += p4.w;
                        }
                        *reinterpret_cast<float4*>(d + 4 * h) = o;
                    }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (gx + k < W) d[k] = a.accumulate ? d[k] + e[k] : e[k];
            }
        }
    }
}

template <int DYL, bool DGRAD>
static int launch_s2(const S2Args& a, int N, int tiles_c, int groups, hipStream_t s) {
    const size_t lds = DGRAD ? S2D_LDS : S2F_LDS;
    if (DGRAD) allow_full_lds<conv_s2_dgrad_kernel<DYL>>();
    else allow_full_lds<conv_s2_fwd_kernel<DYL>>();
    const long long blocks = (long long)N * a.tiles_x * a.tiles_y;
    if (blocks > 0x7fffffffLL || tiles_c > 65535 || groups > 65535) return CD_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)blocks, (unsigned)tiles_c, (unsigned)groups);
    if (DGRAD) hipLaunchKernelGGL((conv_s2_dgrad_kernel<DYL>), grid, dim3(kBlock), lds, s, a);
    else hipLaunchKernelGGL((conv_s2_fwd_kernel<DYL>), grid, dim3(kBlock), lds, s, a);
    return hipGetLastError() == hipSuccess ? CD_OK : CD_ERR_LAUNCH;
}

// ---------------------------------------------------------------- weight gradient
constexpr int S2W_TY = 2, S2W_XR = 2 * S2W_TY + 1, S2W_XCS = S2W_XR * 3 * 16 + 4, S2W_SPX = 16 * S2W_XCS;   // words (2 bf16 pixels each)
constexpr int S2W_DCS = S2W_TY * 16 + 4, S2W_SPD = 64 * S2W_DCS;
constexpr size_t S2W_LDS = (size_t)3 * (S2W_SPX + S2W_SPD) * 4;

struct S2WArgs {
    const float* x; const float* dy; float* packed;
    int x_ctot, x_coff, Cin, dy_ctot, dy_coff, Cout, N, H, W, Ho, Wo, tiles_x, tiles_y, cogs, cigs, zpg;
    size_t g_ws;
};

__global__ __launch_bounds__(kBlock, 2) void conv_s2_wgrad_kernel(const S2WArgs a) {
    constexpr int TY = S2W_TY, XR = S2W_XR, XCS = S2W_XCS, SPX = S2W_SPX, DCS = S2W_DCS, SPD = S2W_SPD;
    extern __shared__ __attribute__((aligned(16))) unsigned s2w_smem[];
    unsigned* s_x = s2w_smem;               // [3 splits][16 ci][XR rows][3 planes: columns 2xo-1, 2xo, 2xo+1][32 pixels]
    unsigned* s_dy = s2w_smem + 3 * SPX;    // [3 splits][64 co][TY rows][32 pixels]

    const int grp = (int)blockIdx.z / a.zpg, cog64 = (int)blockIdx.z - grp * a.zpg, cig = (int)blockIdx.y;
    const int H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo, Cin = a.Cin, Cout = a.Cout;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    const size_t HW = (size_t)H * W, HWo = (size_t)Ho * Wo;
    const int x_c0 = a.x_coff + grp * Cin, dy_c0 = a.dy_coff + grp * Cout;
    const int items = a.N * a.tiles_x * a.tiles_y;
    const bool vec_x = (W & 3) == 0, vec_dy = (Wo & 3) == 0;
    const int cog16 = cog64 * 4 + wid;
    const bool active = cog16 < a.cogs;     // wave-uniform: a 16-channel output tile of the packed layout

    f32x4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int item = (int)blockIdx.x; item < items; item += (int)gridDim.x) {
        const int n = item / (a.tiles_x * a.tiles_y), tile = item - n * (a.tiles_x * a.tiles_y);
        const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int X0 = tx * 32, Y0 = ty * TY;     // output coordinates
        const float* x_n = a.x + ((size_t)n * a.x_ctot + x_c0) * HW;
        const float* dy_n = a.dy + ((size_t)n * a.dy_ctot + dy_c0) * HWo;
        __syncthreads();   // the previous tile is consumed
        // ---- x: unit = (channel, tile row, 4 output pixels): input columns c0 - 1 .. c0 + 7, c0 = 2 (X0 + 4q)
        for (int u = threadIdx.x; u < 16 * XR * 8; u += kBlock) {
            const int q = u & 7, r = (u >> 3) % XR, c = u / (8 * XR);
            const int ch = cig * 16 + c, gy = 2 * Y0 - 1 + r, c0 = 2 * (X0 + 4 * q);
            const bool ok = ch < Cin && (unsigned)gy < (unsigned)H;
            const float* rowp = x_n + (size_t)(ch < Cin ? ch : Cin - 1) * HW + (size_t)((unsigned)gy < (unsigned)H ? gy : 0) * W;
            float v[9];
            if (vec_x) {
                const bool in0 = c0 < W, in1 = c0 + 4 < W;
                const float4 f0 = *reinterpret_cast<const float4*>(rowp + (in0 ? c0 : 0));
                const float4 f1 = *reinterpret_cast<const float4*>(rowp + (in1 ? c0 + 4 : 0));
                const float fm = rowp[(c0 >= 1 && c0 - 1 < W) ? c0 - 1 : 0];
                v[0] = (ok && c0 >= 1 && c0 - 1 < W) ? fm : 0.f;
                v[1] = (ok && in0) ? f0.x : 0.f; v[2] = (ok && in0) ? f0.y : 0.f; v[3] = (ok && in0) ? f0.z : 0.f; v[4] = (ok && in0) ? f0.w : 0.f;
                v[5] = (ok && in1) ? f1.x : 0.f; v[6] = (ok && in1) ? f1.y : 0.f; v[7] = (ok && in1) ? f1.z : 0.f; v[8] = (ok && in1) ? f1.w : 0.f;
            } else {
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    const int gx = c0 - 1 + j;
                    const bool in = (unsigned)gx < (unsigned)W;
                    const float f = rowp[in ? gx : 0];
                    v[j] = (ok && in) ? f : 0.f;
                }
            }
            unsigned* d = s_x + c * XCS + r * 48 + 2 * q;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {   // plane pl holds columns 2xo - 1 + pl
                unsigned h0, m0, l0, h1, m1, l1;
                split_pair(v[pl], v[pl + 2], h0, m0, l0);
                split_pair(v[pl + 4], v[pl + 6], h1, m1, l1);
                *reinterpret_cast<u32x2*>(d + pl * 16) = u32x2{h0, h1};
                *reinterpret_cast<u32x2*>(d + pl * 16 + SPX) = u32x2{m0, m1};
                *reinterpret_cast<u32x2*>(d + pl * 16 + 2 * SPX) = u32x2{l0, l1};
            }
        }
        // ---- dy: unit = (channel, row, 4 pixels)
        for (int u = threadIdx.x; u < 64 * TY * 8; u += kBlock) {
            const int q = u & 7, r = (u >> 3) % TY, c = u / (8 * TY);
            const int ch = cog64 * 64 + c, gy = Y0 + r, gx = X0 + 4 * q;
            const bool ok = ch < Cout && gy < Ho;
            const float* rowp = dy_n + (size_t)(ch < Cout ? ch : Cout - 1) * HWo + (size_t)(gy < Ho ? gy : 0) * Wo;
            float v[4];
            if (vec_dy) {
                const bool in = gx < Wo;
                const float4 f = *reinterpret_cast<const float4*>(rowp + (in ? gx : 0));
                v[0] = (ok && in) ? f.x : 0.f; v[1] = (ok && in) ? f.y : 0.f; v[2] = (ok && in) ? f.z : 0.f; v[3] = (ok && in) ? f.w : 0.f;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool in = gx + j < Wo;
                    const float f = rowp[in ? gx + j : 0];
                    v[j] = (ok && in) ? f : 0.f;
                }
            }
            unsigned h0, m0, l0, h1, m1, l1;
            split_pair(v[0], v[1], h0, m0, l0);
            split_pair(v[2], v[3], h1, m1, l1);
            unsigned* d = s_dy + c * DCS + r * 16 + 2 * q;
            *reinterpret_cast<u32x2*>(d) = u32x2{h0, h1};
            *reinterpret_cast<u32x2*>(d + SPD) = u32x2{m0, m1};
            *reinterpret_cast<u32x2*>(d + 2 * SPD) = u32x2{l0, l1};
        }
        __syncthreads();
        if (!active) continue;
        const unsigned* a_ptr = s_dy + (wid * 16 + li) * DCS + 4 * g;
        const unsigned* b_ptr = s_x + li * XCS + 4 * g;
#pragma unroll 1
        for (int y = 0; y < TY; ++y) {
            bf16x8 av[3], bv[3][3][3];   // [ky][split][kx]
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) av[sp] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(a_ptr + sp * SPD + y * 16));
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int sp = 0; sp < 3; ++sp)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
                        bv[ky][sp][kx] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(b_ptr + sp * SPX + ((2 * y + ky) * 3 + kx) * 16));
#pragma unroll
            for (int p = 0; p < 6; ++p)      // all nine taps between two products of one accumulator
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[SPLIT_PA[p]], bv[t / 3][SPLIT_PB[p]][t % 3], acc[t], 0, 0, 0);
        }
    }

    // ---- flush: this block's slice, packed [split][cog16][cig][tap][16 co][16 ci] (D: lane holds ci = lane & 15, co = 4 (lane >> 4) + {0..3})
    if (!active) return;
    const size_t slice = (size_t)a.cogs * a.cigs * 9 * 256;
    float* base = a.packed + (size_t)grp * a.g_ws + (size_t)blockIdx.x * slice + ((size_t)cog16 * a.cigs + cig) * 9 * 256;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        float* dst = base + ((size_t)t * 16 + 4 * g) * 16 + li;
        dst[0] = acc[t].x; dst[16] = acc[t].y; dst[32] = acc[t].z; dst[48] = acc[t].w;
    }
}

// ---------------------------------------------------------------- 2x2 sub-sampling and its adjoint
// y[n][c][yo][xo] = x[n][coff + c][2yo][2xo]; a thread owns 4 output pixels
__global__ void subsample2_fwd_kernel(const float* __restrict__ x, int ctot, int coff, int C, float* __restrict__ y, int N, int H, int W, int Ho, int Wo) {
    const int wq = (Wo + 3) / 4;
    const size_t total = (size_t)N * C * Ho * wq;
    const bool vin = (W & 3) == 0, vout = (Wo & 3) == 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % wq); size_t r = i / wq;
        const int yo = (int)(r % Ho); r /= Ho;
        const int c = (int)(r % C), n = (int)(r / C);
        const float* src = x + (((size_t)n * ctot + coff + c) * H + 2 * yo) * W + 8 * q;
        float* dst = y + (((size_t)n * C + c) * Ho + yo) * Wo + 4 * q;
        float e[4];
        if (vin && 8 * q + 7 < W) {
            const float4 f0 = *reinterpret_cast<const float4*>(src), f1 = *reinterpret_cast<const float4*>(src + 4);
            e[0] = f0.x; e[1] = f0.z; e[2] = f1.x; e[3] = f1.z;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = (8 * q + 2 * k < W) ? src[2 * k] : 0.f;
        }
        if (vout) *reinterpret_cast<float4*>(dst) = make_float4(e[0], e[1], e[2], e[3]);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < Wo) dst[k] = e[k];
        }
    }
}

// dx[n][coff + c][y][x] = dy[n][c][y/2][x/2] at even (y, x), 0 elsewhere: the whole plane in one pass; a thread owns 4 dx pixels
__global__ void subsample2_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int ctot, int coff, int C, int N, int H, int W, int Ho, int Wo) {
    const int wq = (W + 3) / 4;
    const size_t total = (size_t)N * C * H * wq;
    const bool vout = (W & 3) == 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % wq); size_t r = i / wq;
        const int yy = (int)(r % H); r /= H;
        const int c = (int)(r % C), n = (int)(r / C);
        float* dst = dx + (((size_t)n * ctot + coff + c) * H + yy) * W + 4 * q;
        float e0 = 0.f, e2 = 0.f;
        if ((yy & 1) == 0) {
            const float* src = dy + (((size_t)n * C + c) * Ho + (yy >> 1)) * Wo + 2 * q;
            if (2 * q < Wo) e0 = src[0];
            if (2 * q + 1 < Wo && 4 * q + 2 < W) e2 = src[1];
        }
        if (vout) *reinterpret_cast<float4*>(dst) = make_float4(e0, 0.f, e2, 0.f);
        else {
            const float e[4] = {e0, 0.f, e2, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < W) dst[k] = e[k];
        }
    }
}

static inline bool strided_enabled_arith() { return cd_get_conv_arith() >= 1; }

}  // namespace cd

extern "C" {

int cd_conv2d_strided_supported(int pass, int ks, int stride, int cin_g, int cout_g) {
    if (pass < 0 || pass > 2 || stride != 2 || cin_g <= 0 || cout_g <= 0) return 0;
    if (ks == 1) return 1;                 // cd_subsample2_fwd / _bwd around the stride-1 1x1 entries
    return (ks == 3 && cin_g >= 8) ? 1 : 0;   // (fewer input channels -- the RGB stems -- and k = 5, 7, 11 have no strided kernel)
}

static int s2_check(int pass, const void* p0, const void* p1, const void* p2, int c0_tot, int c0_off, int c0_g, int c1_tot, int c1_off, int c1_g,
                    int groups, int N, int H, int W, int ks, int stride, int cin_g, int cout_g) {
    if (!p0 || !p1 || !p2 || groups <= 0 || c0_g <= 0 || c1_g <= 0 || N <= 0 || H <= 0 || W <= 0) return CD_ERR_INVALID_ARG;
    if (c0_off < 0 || c0_off + groups * c0_g > c0_tot || c1_off < 0 || c1_off + groups * c1_g > c1_tot) return CD_ERR_INVALID_ARG;
    if (ks != 3 || !cd_conv2d_strided_supported(pass, ks, stride, cin_g, cout_g) || !cd::strided_enabled_arith()) return CD_ERR_UNSUPPORTED;
    return CD_OK;
}

int cd_conv2d_fwd_strided(const float* x, int x_ctot, int x_coff, int cin_g, const float* packed_w, size_t packed_group_stride, const float* bias,
                          float* y, int y_ctot, int y_coff, int cout_g, int groups, int accumulate, int N, int H, int W, int ks, int stride,
                          void* stream) {
    const int rc = s2_check(0, x, packed_w, y, x_ctot, x_coff, cin_g, y_ctot, y_coff, cout_g, groups, N, H, W, ks, stride, cin_g, cout_g);
    if (rc != CD_OK) return rc;
    if (groups > 1 && (packed_group_stride < cd_conv2d_packed_weight_floats(cout_g, cin_g, ks, 0) || packed_group_stride % 4)) return CD_ERR_INVALID_ARG;
    cd::S2Args a;
    a.src = x; a.wsp = reinterpret_cast<const cd::u32x4*>(packed_w + cd::fp32_packed_floats(cout_g, cin_g, ks)); a.bias = bias; a.dst = y;
    a.s_ctot = x_ctot; a.s_coff = x_coff; a.IC = cin_g; a.d_ctot = y_ctot; a.d_coff = y_coff; a.OC = cout_g; a.accumulate = accumulate;
    a.H = H; a.W = W; a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2;
    a.tiles_x = (a.Wo + 31) / 32; a.tiles_y = (a.Ho + cd::S2F_TY - 1) / cd::S2F_TY;
    a.g_s = groups > 1 ? cin_g : 0; a.g_d = groups > 1 ? cout_g : 0; a.g_w = groups > 1 ? packed_group_stride / 4 : 0;
    if (cd::split_dy(cout_g) == 2) return cd::launch_s2<2, false>(a, N, 1, groups, (hipStream_t)stream);
    return cd::launch_s2<1, false>(a, N, cd::split_ntiles(cout_g), groups, (hipStream_t)stream);
}

int cd_conv2d_dgrad_strided(const float* dy, int dy_ctot, int dy_coff, int cout_g, const float* packed_wT, size_t packed_group_stride, float* dx,
                            int dx_ctot, int dx_coff, int cin_g, int groups, int accumulate, int N, int H, int W, int ks, int stride,
                            void* stream) {
    const int rc = s2_check(1, dy, packed_wT, dx, dy_ctot, dy_coff, cout_g, dx_ctot, dx_coff, cin_g, groups, N, H, W, ks, stride, cin_g, cout_g);
    if (rc != CD_OK) return rc;
    if (groups > 1 && (packed_group_stride < cd_conv2d_packed_weight_floats(cout_g, cin_g, ks, 1) || packed_group_stride % 4)) return CD_ERR_INVALID_ARG;
    cd::S2Args a;   // the transposed pack is the filter of the logical convolution cout_g -> cin_g
    a.src = dy; a.wsp = reinterpret_cast<const cd::u32x4*>(packed_wT + cd::fp32_packed_floats(cin_g, cout_g, ks)); a.bias = nullptr; a.dst = dx;
    a.s_ctot = dy_ctot; a.s_coff = dy_coff; a.IC = cout_g; a.d_ctot = dx_ctot; a.d_coff = dx_coff; a.OC = cin_g; a.accumulate = accumulate;
    a.H = H; a.W = W; a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2;
    a.tiles_x = (a.Wo + 31) / 32; a.tiles_y = (a.Ho + cd::S2D_TA - 1) / cd::S2D_TA;
    a.g_s = groups > 1 ? cout_g : 0; a.g_d = groups > 1 ? cin_g : 0; a.g_w = groups > 1 ? packed_group_stride / 4 : 0;
    if (cd::split_dy(cin_g) == 2) return cd::launch_s2<2, true>(a, N, 1, groups, (hipStream_t)stream);
    return cd::launch_s2<1, true>(a, N, cd::split_ntiles(cin_g), groups, (hipStream_t)stream);
}

int cd_conv2d_wgrad_strided(const float* x, int x_ctot, int x_coff, int cin_g, const float* dy, int dy_ctot, int dy_coff, int cout_g, int groups,
                            float* dw, int accumulate, float* workspace, size_t workspace_group_stride, int N, int H, int W, int ks, int stride,
                            void* stream) {
    if (!dw) return CD_ERR_INVALID_ARG;
    const int rc = s2_check(2, x, dy, workspace, x_ctot, x_coff, cin_g, dy_ctot, dy_coff, cout_g, groups, N, H, W, ks, stride, cin_g, cout_g);
    if (rc != CD_OK) return rc;
    int cogs, cigs, max_splits;
    size_t slice;
    cd::wgrad_split_layout_info(cout_g, cin_g, ks, &cogs, &cigs, &max_splits, &slice);
    if (groups > 1 && workspace_group_stride < slice * (size_t)max_splits) return CD_ERR_INVALID_ARG;
    cd::S2WArgs a;
    a.x = x; a.dy = dy; a.packed = workspace; a.x_ctot = x_ctot; a.x_coff = x_coff; a.Cin = cin_g; a.dy_ctot = dy_ctot; a.dy_coff = dy_coff;
    a.Cout = cout_g; a.N = N; a.H = H; a.W = W; a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2;
    a.tiles_x = (a.Wo + 31) / 32; a.tiles_y = (a.Ho + cd::S2W_TY - 1) / cd::S2W_TY;
    a.cogs = cogs; a.cigs = cigs; a.zpg = (cogs + 3) / 4; a.g_ws = groups > 1 ? workspace_group_stride : 0;
    if ((long long)a.zpg * groups > 65535 || cigs > 65535) return CD_ERR_UNSUPPORTED;
    // blocks per channel-group pair: about two per compute unit over the whole launch, never more slices than the workspace holds
    const long long items = (long long)N * a.tiles_x * a.tiles_y;
    if (items > 0x7fffffffLL) return CD_ERR_UNSUPPORTED;
    long long splits = 512 / ((long long)a.zpg * cigs * groups);
    if (splits > max_splits) splits = max_splits;
    if (splits > items) splits = items;
    if (splits < 1) splits = 1;
    cd::allow_full_lds<cd::conv_s2_wgrad_kernel>();
    hipLaunchKernelGGL(cd::conv_s2_wgrad_kernel, dim3((unsigned)splits, (unsigned)cigs, (unsigned)(a.zpg * groups)), dim3(cd::kBlock), cd::S2W_LDS,
                       (hipStream_t)stream, a);
    CD_CHECK_LAUNCH();
    return cd::launch_unpack_wgrad_split(workspace, cout_g, cin_g, ks, cigs, (int)splits, slice, dw, accumulate & 1, groups, a.g_ws, (hipStream_t)stream);
}

int cd_subsample2_fwd(const float* x, int ctot, int coff, int C, float* y, int N, int H, int W, void* stream) {
    if (!x || !y || C <= 0 || N <= 0 || H <= 0 || W <= 0 || coff < 0 || coff + C > ctot) return CD_ERR_INVALID_ARG;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const size_t total = (size_t)N * C * Ho * ((Wo + 3) / 4);
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(cd::subsample2_fwd_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, x, ctot, coff, C, y,
                       N, H, W, Ho, Wo);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

int cd_subsample2_bwd(const float* dy, float* dx, int ctot, int coff, int C, int N, int H, int W, void* stream) {
    if (!dy || !dx || C <= 0 || N <= 0 || H <= 0 || W <= 0 || coff < 0 || coff + C > ctot) return CD_ERR_INVALID_ARG;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const size_t total = (size_t)N * C * H * ((W + 3) / 4);
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(cd::subsample2_bwd_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, dy, dx, ctot, coff, C,
                       N, H, W, Ho, Wo);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

}  // extern "C"
