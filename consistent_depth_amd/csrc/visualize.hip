// Colour-mapped previews of inverse depth maps -- the PNGs the reference writes next to every exported `.raw`.
//
// Replaces (reference): utils/visualization.py:20-37 visualize_depth and the range pass of :40-101 visualize_depth_dir --
//     s   = ((d - dmin) / (dmax - dmin)) ** 0.5              float32 throughout; ** 0.5 is sqrt bit for bit
//     idx = uint8(s * 255)                                   low byte of the int32 truncation on x86; 0 for NaN and out-of-int32 values
//     out = rint(((CM_MAGMA[idx] / 255) ** 2.2) * 255)       a fixed 256 x 3 byte table (consistent_depth_amd/utils/magma_gamma22_u8.txt)
//     dmin / dmax = min / max over the files of np.percentile(finite values, q)
// depth_colorize_kernel: memory bound, 4 B in and 3 B out per pixel; the table lives in LDS as one packed dword per entry; a lane
// takes 4 pixels (one 16 B load, one 12 B store); a scalar path covers H*W*N % 4 != 0 and bases that are not 16 B / 4 B aligned.
// depth_range_kernel: one workgroup per plane; percentiles other than 0 / 100 by scale.hip's MSB-first radix select (4 passes of an
// 8-bit LDS histogram per order statistic, one more for its upper neighbour); the plane (0.34 MB at 384x224) is re-read from L2.
// No float atomics: minima and maxima are integer atomics on the order-preserving keys, in LDS.
#include "cd_common.h"
#include "order_key.h"

namespace cd {

constexpr int kRangeThreads = 1024;
constexpr int kColorThreads = 256;

struct SelectShared {
    unsigned hist[256];
    unsigned prefix, k, cle, mingt;
};

// The k-th smallest (0-based) finite value of x[0..HW) and its upper neighbour (the (k+1)-th, or the k-th itself when k is the last),
// as order keys.  n = number of finite values, k < n.  Called by all threads of the workgroup with uniform arguments.
__device__ void select_kth_finite(const float* __restrict__ x, int HW, unsigned k, unsigned n, SelectShared& s, unsigned& key_lo,
                                  unsigned& key_next) {
    const int t = threadIdx.x;
    if (t == 0) { s.prefix = 0u; s.k = k; s.cle = 0u; s.mingt = 0xffffffffu; }
    __syncthreads();
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = t; i < 256; i += kRangeThreads) s.hist[i] = 0u;
        __syncthreads();
        const unsigned prefix = s.prefix;
        for (int p = t; p < HW; p += kRangeThreads) {
            const float v = x[p];
            if (isfinite(v)) {
                const unsigned key = order_key(v);
                if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&s.hist[(key >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        if (t == 0) {
            unsigned kk = s.k, cum = 0u;
            int bin = 0;
            for (; bin < 255; ++bin) {
                if (cum + s.hist[bin] > kk) break;
                cum += s.hist[bin];
            }
            s.k = kk - cum;
            s.prefix = (prefix << 8) | (unsigned)bin;
        }
        __syncthreads();
    }
    key_lo = s.prefix;
    key_next = key_lo;
    if (k + 1u < n) {            // (workgroup-uniform)
        unsigned cle = 0u, mingt = 0xffffffffu;
        for (int p = t; p < HW; p += kRangeThreads) {
            const float v = x[p];
            if (isfinite(v)) {
                const unsigned key = order_key(v);
                if (key <= key_lo) ++cle;
                else mingt = key < mingt ? key : mingt;
            }
        }
        atomicAdd(&s.cle, cle);
        atomicMin(&s.mingt, mingt);
        __syncthreads();
        key_next = s.cle >= k + 2u ? key_lo : s.mingt;
    }
    __syncthreads();             // every thread has read s before the next call resets it
}

__global__ __launch_bounds__(kRangeThreads) void depth_range_kernel(const float* __restrict__ planes, int HW, int mode, float q_lo, float q_hi,
                                                                    int* __restrict__ count_out, float* __restrict__ stats_out) {
    __shared__ SelectShared sel;
    __shared__ unsigned s_n, s_nan, s_min, s_max;
    const int f = blockIdx.x, t = threadIdx.x;
    const float* x = planes + (size_t)f * HW;
    float* stats = stats_out + 4 * (size_t)f;
    const float nanv = __uint_as_float(0x7fc00000u);
    if (t == 0) { s_n = 0u; s_nan = 0u; s_min = 0xffffffffu; s_max = 0u; }
    __syncthreads();
    {
        unsigned n = 0u, nan = 0u, kmin = 0xffffffffu, kmax = 0u;
        for (int p = t; p < HW; p += kRangeThreads) {
            const float v = x[p];
            const bool take = mode == CD_RANGE_NANMAX ? v == v : isfinite(v);
            nan += v != v ? 1u : 0u;
            if (take) {
                const unsigned key = order_key(v);
                ++n;
                kmin = key < kmin ? key : kmin;
                kmax = key > kmax ? key : kmax;
            }
        }
        if (n) { atomicAdd(&s_n, n); atomicMin(&s_min, kmin); atomicMax(&s_max, kmax); }
        if (nan) atomicAdd(&s_nan, nan);
    }
    __syncthreads();
    const unsigned n = s_n;
    if (mode != CD_RANGE_PERCENTILE) {
        if (t == 0) {
            const bool none = mode == CD_RANGE_NANMAX ? s_nan != 0u : n == 0u;
            const float lo = none ? nanv : key_value(s_min), hi = none ? nanv : key_value(s_max);
            count_out[f] = mode == CD_RANGE_NANMAX ? HW : (int)n;
            stats[0] = lo; stats[1] = lo; stats[2] = hi; stats[3] = hi;
        }
        return;
    }
    if (n == 0u) {               // (workgroup-uniform)
        if (t == 0) { count_out[f] = 0; stats[0] = nanv; stats[1] = nanv; stats[2] = nanv; stats[3] = nanv; }
        return;
    }
    if (t == 0) count_out[f] = (int)n;
    for (int which = 0; which < 2; ++which) {
        // numpy: virtual index (n - 1) * q as a float32 product; at or above n - 1 both neighbours are the last element
        const float last = (float)(n - 1u);
        const float vi = __fmul_rn(last, which ? q_hi : q_lo);
        unsigned k = n - 1u;
        if (vi < last) k = (unsigned)floorf(vi);
        unsigned key_lo, key_next;
        select_kth_finite(x, HW, k, n, sel, key_lo, key_next);
        if (t == 0) { stats[2 * which] = key_value(key_lo); stats[2 * which + 1] = key_value(key_next); }
    }
}

__global__ __launch_bounds__(kWave) void depth_range_fold_kernel(const int* __restrict__ counts, const float* __restrict__ stats, int N, int nan_max,
                                                                 float* __restrict__ dmin_out, float* __restrict__ dmax_out) {
    // one wave: lane-strided over the planes, then a shuffle reduction (float compares, no atomics)
    const int t = threadIdx.x;
    float lo = __uint_as_float(0x7f800000u), hi = nan_max ? __uint_as_float(0xff800000u) : 0.f;
    bool nan = false;
    for (int i = t; i < N; i += kWave) {
        if (!nan_max && counts[i] <= 0) continue;
        const float a = stats[4 * i], b = stats[4 * i + 3];
        nan = nan || a != a || b != b;
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const float a = __shfl_down(lo, off, kWave), b = __shfl_down(hi, off, kWave);
        const int o = __shfl_down((int)nan, off, kWave);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
        nan = nan || o != 0;
    }
    if (t == 0) {
        const float nanv = __uint_as_float(0x7fc00000u);
        *dmin_out = (nan_max && nan) ? nanv : lo;
        *dmax_out = (nan_max && nan) ? nanv : hi;
    }
}

__device__ __forceinline__ unsigned colour_of(float d, float dmin, float den, const unsigned* lut) {
    const float v = __fmul_rn(__fsqrt_rn(__fdiv_rn(__fsub_rn(d, dmin), den)), 255.f);
    // v_cvt_i32_f32 saturates; the reference's conversion yields 0 for NaN and for values outside int32
    const unsigned idx = fabsf(v) < 2147483648.f ? ((unsigned)(int)v & 255u) : 0u;
    return lut[idx];
}

struct __attribute__((aligned(4))) Rgb4 { unsigned w0, w1, w2; };     // 4 pixels x 3 bytes

__global__ __launch_bounds__(kColorThreads) void depth_colorize_kernel(const float* __restrict__ d, size_t total, const float* __restrict__ dmin_p,
                                                                       const float* __restrict__ dmax_p, const unsigned char* __restrict__ table,
                                                                       int bgr, unsigned char* __restrict__ out, int vec) {
    __shared__ unsigned lut[256];        // byte 0 = first channel written, byte 2 = last
    for (int i = threadIdx.x; i < 256; i += kColorThreads) {
        const unsigned r = table[3 * i], g = table[3 * i + 1], b = table[3 * i + 2];
        lut[i] = bgr ? (b | (g << 8) | (r << 16)) : (r | (g << 8) | (b << 16));
    }
    __syncthreads();
    const float dmin = *dmin_p, den = __fsub_rn(*dmax_p, dmin);
    const size_t gtid = (size_t)blockIdx.x * kColorThreads + threadIdx.x, stride = (size_t)gridDim.x * kColorThreads;
    const size_t groups = vec ? total / 4 : 0;
    for (size_t g = gtid; g < groups; g += stride) {
        const float4 v = reinterpret_cast<const float4*>(d)[g];
        const unsigned c0 = colour_of(v.x, dmin, den, lut), c1 = colour_of(v.y, dmin, den, lut);
        const unsigned c2 = colour_of(v.z, dmin, den, lut), c3 = colour_of(v.w, dmin, den, lut);
        Rgb4 o;
        o.w0 = c0 | (c1 << 24);
        o.w1 = (c1 >> 8) | (c2 << 16);
        o.w2 = (c2 >> 16) | (c3 << 8);
        reinterpret_cast<Rgb4*>(out)[g] = o;
    }
    for (size_t p = groups * 4 + gtid; p < total; p += stride) {
        const unsigned c = colour_of(d[p], dmin, den, lut);
        out[3 * p] = (unsigned char)(c & 255u);
        out[3 * p + 1] = (unsigned char)((c >> 8) & 255u);
        out[3 * p + 2] = (unsigned char)((c >> 16) & 255u);
    }
}

}  // namespace cd

static bool plane_args_ok(const void* planes, int N, int H, int W) {
    return planes && N > 0 && H > 0 && W > 0 && (long long)H * W <= (1ll << 30) && (long long)N * H * W <= (1ll << 40);
}

extern "C" int cd_depth_range(const float* planes, int N, int H, int W, int mode, float q_lo, float q_hi, int* count_out, float* stats_out,
                              void* stream) {
    if (!plane_args_ok(planes, N, H, W) || !count_out || !stats_out || mode < CD_RANGE_MINMAX || mode > CD_RANGE_NANMAX) return CD_ERR_INVALID_ARG;
    if (mode == CD_RANGE_PERCENTILE && !(q_lo >= 0.f && q_lo <= 1.f && q_hi >= 0.f && q_hi <= 1.f)) return CD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(cd::depth_range_kernel, dim3(N), dim3(cd::kRangeThreads), 0, (hipStream_t)stream, planes, H * W, mode, q_lo, q_hi, count_out,
                       stats_out);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

extern "C" int cd_depth_range_fold(const int* counts, const float* stats, int N, int nan_max, float* dmin_out, float* dmax_out, void* stream) {
    if (!counts || !stats || N <= 0 || !dmin_out || !dmax_out) return CD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(cd::depth_range_fold_kernel, dim3(1), dim3(cd::kWave), 0, (hipStream_t)stream, counts, stats, N, nan_max ? 1 : 0, dmin_out,
                       dmax_out);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

extern "C" int cd_depth_colorize(const float* planes, int N, int H, int W, const float* dmin, const float* dmax, const unsigned char* table,
                                 int bgr, unsigned char* out, void* stream) {
    if (!plane_args_ok(planes, N, H, W) || !dmin || !dmax || !table || !out || ((uintptr_t)planes & 3u)) return CD_ERR_INVALID_ARG;
    const size_t total = (size_t)N * H * W;
    const int vec = (((uintptr_t)planes & 15u) == 0 && ((uintptr_t)out & 3u) == 0) ? 1 : 0;
    const size_t items = vec ? (total + 3) / 4 : total;
    size_t blocks = (items + cd::kColorThreads - 1) / cd::kColorThreads;
    if (blocks > 4096) blocks = 4096;          // grid-stride beyond: 16 blocks per CU
    hipLaunchKernelGGL(cd::depth_colorize_kernel, dim3((unsigned)blocks), dim3(cd::kColorThreads), 0, (hipStream_t)stream, planes, total, dmin, dmax,
                       table, bgr ? 1 : 0, out, vec);
    CD_CHECK_LAUNCH();
    return CD_OK;
}
