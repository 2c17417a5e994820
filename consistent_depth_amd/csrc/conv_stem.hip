// The 7x7 / 2 RGB stem -- nn.Conv2d(Cin <= 4, Cout, 7, stride 2, padding 3) -- at fp32 accuracy on the gfx950 BF16 matrix cores:
// forward and weight gradient (the input gradient of an image is never asked for; see ops/conv_layer.py).
//
// Geometry: input H x W, output Ho x Wo = ceil(H/2) x ceil(W/2); output pixel (yo, xo) reads input rows 2yo - 3 .. 2yo + 3 and
// columns 2xo - 3 .. 2xo + 3, zeros outside.  Arithmetic: the split-bf16 scheme of split_bf16.h (three exact bf16 terms per
// operand, six cross products, smallest first, fp32 accumulation).  No atomics, no allocation; the order of accumulation depends
// on the shape only.
//
// With 3 input channels a channel tile has nothing to reduce over, so the reduction index of both GEMMs is the FLATTENED tap
// k = (ci * 7 + ky) * 7 + kx -- the memory order of the plain [Cout][Cin][7][7] filter, which the kernels read directly (no packed
// filter) -- padded with zero columns to the MFMA step: K = 147 -> 160 at Cin = 3.
//
// The input tile is staged ONCE per work item as fp32, de-interleaved by column parity: per (channel, row) an even-column and an
// odd-column run of STEM_PW words.  Output pixel X0 + i and tap kx meet tile column 2i + kx + 1, i.e. word i + (kx + 1) / 2 of the
// run of parity (kx + 1) & 1: for a fixed tap the 32 pixels of an M tile are 32 CONSECUTIVE words (forward: a conflict-free
// ds_read_b32 per tap), and for a fixed tap 8 consecutive pixels are 8 consecutive words (weight gradient).  Fragments are split
// in registers after the gather (split8).
//
// Forward (conv_stem_s2_fwd_kernel): implicit GEMM M = 32 output pixels of a row, N = 32 output channels, K = 16 taps per
// v_mfma_f32_32x32x16_bf16.  A workgroup splits its 32 NT output channels of the filter into LDS once ([step][tile][split][lane]
// 16-byte fragments) and walks 8 x 32 output tiles grid-stride; a wave owns two rows of a tile and NT column tiles.
//
// Weight gradient (conv_stem_s2_wgrad_kernel): GEMM M = 32 output channels, N = 32 taps, K = 16 output pixels of a row; dy is read at
// its own resolution.  A wave owns one row of a 4 x 32 tile and all 32 MT x KP accumulators; a workgroup walks tiles grid-stride, adds its
// four waves in wave order through LDS and writes ONE slice [co][KP] of the caller's workspace.  conv_stem_wgrad_reduce_kernel adds the
// slices in a fixed order (16 interleaved chains per element, then those 16 in order): bit-reproducible.
#include "cd_common.h"
#include "conv_stem_map.h"
#include "split_bf16.h"

namespace cd {

constexpr int STEM_MAX_SPLITS = 512;   // slices of the weight-gradient workspace

// split8 for a fragment that feeds an MFMA straight from registers.  Its conversions are inline assembly, which the compiler does not
// see as vector instructions: it pads no wait states between them and a matrix instruction that reads their result (two are needed on
// gfx950; without them the forward kernel read stale fragment registers).  The statement below orders the three fragments before two idle
// states; every MFMA operand of this file comes through here.
__device__ __forceinline__ void stem_split8(const float (&v)[8], bf16x8 (&f)[3]) {
    split8(v, f);
    asm volatile("s_nop 1" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]));
}

// Stage the `ROWS` x 72 input tile of CIN channels whose first element is input (gy0, gx0), gx0 a multiple of 4: zeros outside.
template <int CIN, int ROWS>
__device__ __forceinline__ void stem_stage_x(float* s_x, const float* xin, int gy0, int gx0, int H, int W) {
    constexpr int QUADS = STEM_RS / 4;
    const size_t HW = (size_t)H * W;
    const bool vec_in = (W & 3) == 0;
    for (int u = threadIdx.x; u < CIN * ROWS * QUADS; u += kBlock) {
        const int q = u % QUADS, r = (u / QUADS) % ROWS, ci = u / (QUADS * ROWS);
        const int gy = gy0 + r, gx = gx0 + 4 * q;
        const bool row_in = (unsigned)gy < (unsigned)H;
        const float* rowp = xin + (size_t)ci * HW + (size_t)(row_in ? gy : 0) * W;
        float v[4];
        if (vec_in) {       // W % 4 == 0: an aligned quad is inside or outside the image as a whole
            const bool in = row_in && (unsigned)gx < (unsigned)W;
            const float4 f = *reinterpret_cast<const float4*>(rowp + (in ? gx : 0));
            v[0] = in ? f.x : 0.f; v[1] = in ? f.y : 0.f; v[2] = in ? f.z : 0.f; v[3] = in ? f.w : 0.f;
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const bool in = row_in && (unsigned)(gx + p) < (unsigned)W;
                const float f = rowp[in ? gx + p : 0];
                v[p] = in ? f : 0.f;
            }
        }
        float* d = s_x + stem_tile_word(ci, r, 4 * q, ROWS);     // tile columns 4q, 4q + 2 -> even run, 4q + 1, 4q + 3 -> odd run
        *reinterpret_cast<float2*>(d) = make_float2(v[0], v[2]);
        *reinterpret_cast<float2*>(d + STEM_PW) = make_float2(v[1], v[3]);
    }
}

// ---------------------------------------------------------------- forward
struct StemArgs {
    const float* x; const float* w; const float* bias; float* y;
    int x_ctot, x_coff, y_ctot, y_coff, Cout, N, H, W, Ho, Wo, tiles_x, tiles_y;
};

__host__ __device__ constexpr size_t sf_lds(int cin, int nt) { return ((size_t)cin * SF_ROWS * STEM_RS + (size_t)sf_ksteps(cin) * nt * 3 * 64 * 4) * 4; }

template <int CIN, int NT>
__global__ __launch_bounds__(kBlock, 2) void conv_stem_s2_fwd_kernel(const StemArgs a) {
    constexpr int K = stem_k(CIN), KSTEPS = sf_ksteps(CIN), ROWS = SF_ROWS, XW = CIN * ROWS * STEM_RS;
    extern __shared__ __attribute__((aligned(16))) unsigned char stem_smem[];
    float* s_x = reinterpret_cast<float*>(stem_smem);              // [CIN][ROWS][parity][STEM_PW] fp32
    u32x4* s_w = reinterpret_cast<u32x4*>(stem_smem + (size_t)XW * 4);   // [KSTEPS][NT][3 splits][64 lanes] B fragments

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, li = lane & 31, g = lane >> 5;
    const int H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo, Cout = a.Cout;
    const int co_base = (int)blockIdx.y * (NT * 32);

    // ---- the filter of this block's output channels, split once: fragment (step, tile, lane) = taps 16 st + 8 (lane >> 5) + {0..7}
    for (int f = threadIdx.x; f < KSTEPS * NT * 64; f += kBlock) {
        const int ln = f & 63, nt = (f >> 6) % NT, st = f / (64 * NT);
        const int co = co_base + nt * 32 + (ln & 31), k0 = st * 16 + 8 * (ln >> 5);
        const float* wr = a.w + (size_t)(co < Cout ? co : Cout - 1) * K;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool ok = co < Cout && k0 + j < K;
            const float t = wr[ok ? k0 + j : 0];
            v[j] = ok ? t : 0.f;         // zero columns pad K, zero rows pad Cout
        }
        bf16x8 fr[3];
        split8(v, fr);
#pragma unroll
        for (int sp = 0; sp < 3; ++sp) s_w[((st * NT + nt) * 3 + sp) * 64 + ln] = __builtin_bit_cast(u32x4, fr[sp]);
    }

    const int tiles_img = a.tiles_x * a.tiles_y, items = a.N * tiles_img;
    for (int item = (int)blockIdx.x; item < items; item += (int)gridDim.x) {
        const int n = item / tiles_img, t_lin = item - n * tiles_img;
        const int ty = t_lin / a.tiles_x, tx = t_lin - ty * a.tiles_x;
        const int X0 = tx * 32, Y0 = ty * SF_TY;                   // output coordinates
        __syncthreads();   // the previous tile is consumed
        stem_stage_x<CIN, ROWS>(s_x, a.x + ((size_t)n * a.x_ctot + a.x_coff) * H * W, 2 * Y0 - 3, 2 * X0 - 4, H, W);
        __syncthreads();

        f32x16 acc[2][NT];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[m][nt][q] = 0.f;

#pragma unroll
        for (int st = 0; st < KSTEPS; ++st) {
            bf16x8 av[2][3], b[NT][3];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int sp = 0; sp < 3; ++sp) b[nt][sp] = __builtin_bit_cast(bf16x8, s_w[((st * NT + nt) * 3 + sp) * 64 + lane]);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const float* p = s_x + 2 * (wid + 4 * m) * STEM_RS + li;
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k0 = 16 * st + j, k1 = k0 + 8;       // the tap of lane half 0 / 1 (compile-time after unrolling)
                    const bool v0 = k0 < K, v1 = k1 < K;
                    const int off = g ? (v1 ? stem_off(k1, ROWS) : 0) : (v0 ? stem_off(k0, ROWS) : 0);
                    float t = p[off];
                    if (!(v0 && v1)) t = (g ? v1 : v0) ? t : 0.f;   // a padding column is an exact zero
                    v[j] = t;
                }
                stem_split8(v, av[m]);
            }
#pragma unroll
            for (int pr = 0; pr < 6; ++pr)
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[m][SPLIT_PA[pr]], b[nt][SPLIT_PB[pr]], acc[m][nt], 0, 0, 0);
        }

        // ---- epilogue.  D: lane holds channel lane & 31, pixels 8q + 4g + {0..3}
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int co = co_base + nt * 32 + li;
            if (co >= Cout) continue;
            const float bv = a.bias != nullptr ? a.bias[co] : 0.f;
            float* yout = a.y + ((size_t)n * a.y_ctot + a.y_coff + co) * Ho * Wo;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int gy = Y0 + wid + 4 * m;
                if (gy >= Ho) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int gx = X0 + 8 * q + 4 * g;
                    const float e[4] = {acc[m][nt][4 * q] + bv, acc[m][nt][4 * q + 1] + bv, acc[m][nt][4 * q + 2] + bv, acc[m][nt][4 * q + 3] + bv};
                    float* d = yout + (size_t)gy * Wo + gx;
                    if ((Wo & 3) == 0) {
                        if (gx < Wo) *reinterpret_cast<float4*>(d) = make_float4(e[0], e[1], e[2], e[3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (gx + k < Wo) d[k] = e[k];
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------- weight gradient
struct StemWArgs {
    const float* x; const float* dy; float* ws;
    int x_ctot, x_coff, dy_ctot, dy_coff, Cout, N, H, W, Ho, Wo, tiles_x, tiles_y, copad;
};

constexpr int SW_DS = 36;   // dy rows of 32 pixels, padded: 16-byte reads of 32 channels tile the banks
__host__ __device__ constexpr size_t sw_lds(int cin, int mt) { return ((size_t)cin * SW_ROWS * STEM_RS + (size_t)SW_TY * mt * 32 * SW_DS) * 4; }

template <int CIN, int MT>
__global__ __launch_bounds__(kBlock, (MT * (stem_kp(CIN) / 32) * 16 <= 128) ? 2 : 1) void conv_stem_s2_wgrad_kernel(const StemWArgs a) {
    constexpr int K = stem_k(CIN), KP = stem_kp(CIN), NTL = KP / 32, ROWS = SW_ROWS, XW = CIN * ROWS * STEM_RS, DS = SW_DS, CO = MT * 32;
    static_assert(sw_lds(CIN, MT) >= (size_t)4 * 16 * 64 * 4, "the tiles' LDS also holds the four waves' copies of one accumulator tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char stem_smem[];
    float* s_x = reinterpret_cast<float*>(stem_smem);   // [CIN][ROWS][parity][STEM_PW]
    float* s_dy = s_x + XW;                             // [SW_TY rows][CO channels][DS]

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, li = lane & 31, g = lane >> 5;
    const int H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo, Cout = a.Cout;
    const int co_base = (int)blockIdx.y * CO;
    const size_t HWo = (size_t)Ho * Wo;
    const bool vec_dy = (Wo & 3) == 0;

    // this lane's tap of every column tile: LDS word relative to (tile row 2y, word i), and whether it is a real tap
    int toff[NTL];
    bool tlive[NTL];
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt) {
        const int k = nt * 32 + li;
        tlive[nt] = k < K;
        toff[nt] = tlive[nt] ? stem_off(k, ROWS) : 0;
    }

    f32x16 acc[MT][NTL];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[m][nt][q] = 0.f;

    const int tiles_img = a.tiles_x * a.tiles_y, items = a.N * tiles_img;
    for (int item = (int)blockIdx.x; item < items; item += (int)gridDim.x) {
        const int n = item / tiles_img, t_lin = item - n * tiles_img;
        const int ty = t_lin / a.tiles_x, tx = t_lin - ty * a.tiles_x;
        const int X0 = tx * 32, Y0 = ty * SW_TY;                   // output coordinates
        const float* dy_n = a.dy + ((size_t)n * a.dy_ctot + a.dy_coff) * HWo;
        __syncthreads();   // the previous tile is consumed
        stem_stage_x<CIN, ROWS>(s_x, a.x + ((size_t)n * a.x_ctot + a.x_coff) * H * W, 2 * Y0 - 3, 2 * X0 - 4, H, W);
        // ---- dy: unit = (channel, row, 4 pixels); zeros beyond Cout / Ho / Wo
        for (int u = threadIdx.x; u < CO * SW_TY * 8; u += kBlock) {
            const int q = u & 7, r = (u >> 3) % SW_TY, c = u / (8 * SW_TY);
            const int ch = co_base + c, gy = Y0 + r, gx = X0 + 4 * q;
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
            *reinterpret_cast<float4*>(s_dy + (r * CO + c) * DS + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();

        // ---- this wave's row of the tile: two K steps of 16 output pixels
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            bf16x8 av[MT][3];
#pragma unroll
            for (int m = 0; m < MT; ++m) {     // A: dy[channel 32 m + li][pixels 16 h + 8 g + {0..7}]
                const float* p = s_dy + (wid * CO + m * 32 + li) * DS + 16 * h + 8 * g;
                const float4 f0 = *reinterpret_cast<const float4*>(p), f1 = *reinterpret_cast<const float4*>(p + 4);
                const float v[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
                stem_split8(v, av[m]);
            }
            const float* xb = s_x + 2 * wid * STEM_RS + 16 * h + 8 * g;
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt) {     // B: x under tap 32 nt + li at the same 8 pixels: 8 consecutive words of a parity run
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float t = xb[toff[nt] + j];
                    v[j] = tlive[nt] ? t : 0.f;
                }
                bf16x8 bv[3];
                stem_split8(v, bv);
#pragma unroll
                for (int pr = 0; pr < 6; ++pr)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[m][SPLIT_PA[pr]], bv[SPLIT_PB[pr]], acc[m][nt], 0, 0, 0);
            }
        }
    }

    // ---- flush: the four waves of every accumulator tile added in wave order, into this block's slice [copad][KP].
    // D: lane holds tap lane & 31, channels (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); a thread owns 4 consecutive taps of one register
    float* red = reinterpret_cast<float*>(stem_smem);   // [4 waves][16 registers][64 lanes]
    float* slice = a.ws + (size_t)blockIdx.x * a.copad * KP;
    const int reg = threadIdx.x >> 4, l0 = (threadIdx.x & 15) * 4;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) red[(wid * 16 + r) * 64 + lane] = acc[m][nt][r];
            __syncthreads();
            float4 s = *reinterpret_cast<const float4*>(red + threadIdx.x * 4);
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float4 o = *reinterpret_cast<const float4*>(red + w * 1024 + threadIdx.x * 4);
                s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
            }
            const int co = co_base + m * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (l0 >> 5);
            *reinterpret_cast<float4*>(slice + (size_t)co * KP + nt * 32 + (l0 & 31)) = s;
        }
}

// dw[co][k] (+)= the slices of element (co, k): 16 interleaved chains (slice s, s + 16, ...), then the 16 chains in order
__global__ __launch_bounds__(kBlock) void conv_stem_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int total, int K, int KP,
                                                                        int copad, int splits, int accumulate) {
    __shared__ float part[16][17];
    const int oi = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int o = (int)blockIdx.x * 16 + oi;
    float s = 0.f;
    if (o < total) {
        const int co = o / K, k = o - co * K;
        const float* p = ws + (size_t)co * KP + k;
        for (int sp = sl; sp < splits; sp += 16) s += p[(size_t)sp * copad * KP];
    }
    part[sl][oi] = s;
    __syncthreads();
    if (sl == 0 && o < total) {
        float t = part[0][oi];
#pragma unroll
        for (int i = 1; i < 16; ++i) t += part[i][oi];
        dw[o] = accumulate ? dw[o] + t : t;
    }
}

template <int CIN, int NT>
static int launch_stem_fwd(const StemArgs& a, int co_blocks, hipStream_t s) {
    allow_full_lds<conv_stem_s2_fwd_kernel<CIN, NT>>();
    const long long items = (long long)a.N * a.tiles_x * a.tiles_y;
    if (items > 0x7fffffffLL || co_blocks > 65535) return CD_ERR_UNSUPPORTED;
    const unsigned blocks = (unsigned)(items < 512 ? items : 512);     // two workgroups per compute unit, tiles grid-stride
    hipLaunchKernelGGL((conv_stem_s2_fwd_kernel<CIN, NT>), dim3(blocks, (unsigned)co_blocks), dim3(kBlock), sf_lds(CIN, NT), s, a);
    return hipGetLastError() == hipSuccess ? CD_OK : CD_ERR_LAUNCH;
}

template <int CIN, int MT>
static int launch_stem_wgrad(const StemWArgs& a, int co_blocks, int splits, hipStream_t s) {
    allow_full_lds<conv_stem_s2_wgrad_kernel<CIN, MT>>();
    hipLaunchKernelGGL((conv_stem_s2_wgrad_kernel<CIN, MT>), dim3((unsigned)splits, (unsigned)co_blocks), dim3(kBlock), sw_lds(CIN, MT), s, a);
    return hipGetLastError() == hipSuccess ? CD_OK : CD_ERR_LAUNCH;
}

static int stem_check(int pass, const void* p0, const void* p1, const void* p2, int c0_tot, int c0_off, int c0, int c1_tot, int c1_off, int c1, int N,
                      int H, int W, int ks, int stride, int cin, int cout) {
    if (!p0 || !p1 || !p2 || c0 <= 0 || c1 <= 0 || N <= 0 || H <= 0 || W <= 0) return CD_ERR_INVALID_ARG;
    if (c0_off < 0 || c0_off + c0 > c0_tot || c1_off < 0 || c1_off + c1 > c1_tot) return CD_ERR_INVALID_ARG;
    if (!cd_conv2d_stem_supported(pass, ks, stride, cin, cout) || cd_get_conv_arith() < 1) return CD_ERR_UNSUPPORTED;
    return CD_OK;
}

}  // namespace cd

#define CD_STEM_BY_CIN(cin, CALL)        \
    switch (cin) {                       \
        case 1: return CALL(1);          \
        case 2: return CALL(2);          \
        case 3: return CALL(3);          \
        default: return CALL(4);         \
    }

extern "C" {

int cd_conv2d_stem_supported(int pass, int ks, int stride, int cin, int cout) {
    return ((pass == 0 || pass == 2) && ks == 7 && stride == 2 && cin >= 1 && cin <= 4 && cout >= 8) ? 1 : 0;
}

size_t cd_conv2d_stem_wgrad_workspace_floats(int cout, int cin, int ks) {
    if (ks != 7 || cin < 1 || cin > 4 || cout < 8) return 0;
    const int co_blocks = cout <= 32 ? 1 : (cout + 63) / 64;
    const int splits = cd::STEM_MAX_SPLITS / co_blocks > 0 ? cd::STEM_MAX_SPLITS / co_blocks : 1;
    return (size_t)splits * cd::stem_copad(cout) * cd::stem_kp(cin);
}

int cd_conv2d_stem_fwd(const float* x, int x_ctot, int x_coff, int cin, const float* w, const float* bias, float* y, int y_ctot, int y_coff, int cout,
                       int N, int H, int W, int ks, int stride, void* stream) {
    const int rc = cd::stem_check(0, x, w, y, x_ctot, x_coff, cin, y_ctot, y_coff, cout, N, H, W, ks, stride, cin, cout);
    if (rc != CD_OK) return rc;
    cd::StemArgs a;
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.x_ctot = x_ctot; a.x_coff = x_coff; a.y_ctot = y_ctot; a.y_coff = y_coff; a.Cout = cout;
    a.N = N; a.H = H; a.W = W; a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2;
    a.tiles_x = (a.Wo + 31) / 32; a.tiles_y = (a.Ho + cd::SF_TY - 1) / cd::SF_TY;
    hipStream_t s = (hipStream_t)stream;
    if (cout <= 32) {
#define CD_STEM_CALL(C) cd::launch_stem_fwd<C, 1>(a, 1, s)
        CD_STEM_BY_CIN(cin, CD_STEM_CALL)
#undef CD_STEM_CALL
    }
    const int co_blocks = (cout + 63) / 64;
#define CD_STEM_CALL(C) cd::launch_stem_fwd<C, 2>(a, co_blocks, s)
    CD_STEM_BY_CIN(cin, CD_STEM_CALL)
#undef CD_STEM_CALL
}

int cd_conv2d_stem_wgrad(const float* x, int x_ctot, int x_coff, int cin, const float* dy, int dy_ctot, int dy_coff, int cout, float* dw,
                         float* workspace, int accumulate, int N, int H, int W, int ks, int stride, void* stream) {
    if (!dw) return CD_ERR_INVALID_ARG;
    const int rc = cd::stem_check(2, x, dy, workspace, x_ctot, x_coff, cin, dy_ctot, dy_coff, cout, N, H, W, ks, stride, cin, cout);
    if (rc != CD_OK) return rc;
    cd::StemWArgs a;
    a.x = x; a.dy = dy; a.ws = workspace; a.x_ctot = x_ctot; a.x_coff = x_coff; a.dy_ctot = dy_ctot; a.dy_coff = dy_coff; a.Cout = cout;
    a.N = N; a.H = H; a.W = W; a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2;
    a.tiles_x = (a.Wo + 31) / 32; a.tiles_y = (a.Ho + cd::SW_TY - 1) / cd::SW_TY;
    a.copad = cd::stem_copad(cout);
    const int co_blocks = cout <= 32 ? 1 : (cout + 63) / 64;
    const long long items = (long long)N * a.tiles_x * a.tiles_y;
    if (items > 0x7fffffffLL || co_blocks > 65535) return CD_ERR_UNSUPPORTED;
    // slices: about two workgroups per compute unit over the whole launch, never more than the workspace holds; a function of the shape only
    long long splits = cd::STEM_MAX_SPLITS / co_blocks;
    if (splits < 1) splits = 1;
    if (splits > items) splits = items;
    hipStream_t s = (hipStream_t)stream;
    int lrc;
    if (cout <= 32) {
        switch (cin) {
            case 1: lrc = cd::launch_stem_wgrad<1, 1>(a, 1, (int)splits, s); break;
            case 2: lrc = cd::launch_stem_wgrad<2, 1>(a, 1, (int)splits, s); break;
            case 3: lrc = cd::launch_stem_wgrad<3, 1>(a, 1, (int)splits, s); break;
            default: lrc = cd::launch_stem_wgrad<4, 1>(a, 1, (int)splits, s); break;
        }
    } else {
        switch (cin) {
            case 1: lrc = cd::launch_stem_wgrad<1, 2>(a, co_blocks, (int)splits, s); break;
            case 2: lrc = cd::launch_stem_wgrad<2, 2>(a, co_blocks, (int)splits, s); break;
            case 3: lrc = cd::launch_stem_wgrad<3, 2>(a, co_blocks, (int)splits, s); break;
            default: lrc = cd::launch_stem_wgrad<4, 2>(a, co_blocks, (int)splits, s); break;
        }
    }
    if (lrc != CD_OK) return lrc;
    const int K = cd::stem_k(cin), total = cout * K;
    hipLaunchKernelGGL(cd::conv_stem_wgrad_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(cd::kBlock), 0, s, workspace, dw, total, K,
                       cd::stem_kp(cin), a.copad, (int)splits, accumulate & 1);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

}  // extern "C"
