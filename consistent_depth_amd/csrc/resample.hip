// The memory-bound pieces of the monodepth2 step (KITTI preset) around the MFMA convolutions: bicubic resizing (forward and its
// adjoint), the decoder's input assembly (nearest x2 + skip concat + reflection pad 1) and the crop + activation after a
// "same"-padded convolution of the padded tensor.  fp32 NCHW, no atomics: every backward is a gather with a fixed summation order,
// so it is bit-reproducible.  Each thread produces four consecutive outputs of one row and stores them as one 16-byte store where
// the row length and the base pointer allow it.
//
// Pad-conv-crop: a 3x3 convolution with zero padding 1 applied to reflect_pad1(x) (H+2 x W+2) and restricted to its interior is
// exactly Conv2d(3x3, padding 0)(reflect_pad1(x)).  Its input and weight gradients, fed a gradient that is zero on the ring, are the
// adjoints of that valid convolution, and the bias gradient is the interior sum -- so the tuned "same" convolution kernels serve
// the ReflectionPad2d + Conv2d of monodepth2's decoder unchanged.
#include "cd_common.h"

namespace cd {

struct Tap4 {      // one output index of a bicubic axis: the four (clamped) source indices and their weights
    int i[4];
    float w[4];
};
struct InvTap {    // one entry of the inverted table: an output index and the summed weight it gives this input index
    int o;
    float w;
};

__device__ __forceinline__ bool vec_ok(const float* p, int L) { return (L & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ void store4(float* row, int x0, int L, const float v[4], bool vec) {
    if (vec) {
        *reinterpret_cast<float4*>(row + x0) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (x0 + k < L) row[x0 + k] = v[k];
}

// ---------------------------------------------------------------- bicubic resize (ATen, align_corners=False, explicit size)
// y[nc, oy, ox] = sum_r wy[r] * (sum_j wx[j] * x[nc, iy_r, ix_j])   (x first, then y; left-to-right like ATen's cubic_interp1d)
// then optionally (y - sub) / div.
__global__ __launch_bounds__(kBlock) void bicubic_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int Hin, int Win,
                                                             int Hout, int Wout, const Tap4* __restrict__ ytab,
                                                             const Tap4* __restrict__ xtab, int norm, float sub, float div) {
    const int groups = (Wout + 3) >> 2;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= Hout * groups) return;
    const int oy = t / groups, ox0 = (t - oy * groups) * 4;
    const size_t nc = blockIdx.y;
    const float* src = x + nc * Hin * Win;
    float* dst = y + (nc * Hout + oy) * Wout;
    const Tap4 ty = ytab[oy];
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ox = min(ox0 + k, Wout - 1);
        const Tap4 tx = xtab[ox];
        float rows[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* s = src + (size_t)ty.i[r] * Win;
            rows[r] = s[tx.i[0]] * tx.w[0] + s[tx.i[1]] * tx.w[1] + s[tx.i[2]] * tx.w[2] + s[tx.i[3]] * tx.w[3];
        }
        float v = rows[0] * ty.w[0] + rows[1] * ty.w[1] + rows[2] * ty.w[2] + rows[3] * ty.w[3];
        if (norm) v = (v - sub) / div;
        out[k] = v;
    }
    store4(dst, ox0, Wout, out, vec_ok(y, Wout));
}

// adjoint, pass 1 (x): t[nc, oy, ix] = sum over inv_x[ix] of dy[nc, oy, o] * w
__global__ __launch_bounds__(kBlock) void bicubic_bwd_x_kernel(const float* __restrict__ dy, float* __restrict__ tmp, int Hout,
                                                               int Wout, int Win, const int* __restrict__ xoff,
                                                               const InvTap* __restrict__ xent) {
    const int groups = (Win + 3) >> 2;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= Hout * groups) return;
    const int oy = t / groups, ix0 = (t - oy * groups) * 4;
    const size_t nc = blockIdx.y;
    const float* g = dy + (nc * Hout + oy) * Wout;
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ix = min(ix0 + k, Win - 1);
        float s = 0.f;
        for (int e = xoff[ix]; e < xoff[ix + 1]; ++e) s += g[xent[e].o] * xent[e].w;
        out[k] = s;
    }
    store4(tmp + (nc * Hout + oy) * Win, ix0, Win, out, vec_ok(tmp, Win));
}

// adjoint, pass 2 (y): dx[nc, iy, ix] = sum over inv_y[iy] of t[nc, o, ix] * w   (four consecutive ix per thread: 16-byte loads)
__global__ __launch_bounds__(kBlock) void bicubic_bwd_y_kernel(const float* __restrict__ tmp, float* __restrict__ dx, int Hout,
                                                               int Hin, int Win, const int* __restrict__ yoff,
                                                               const InvTap* __restrict__ yent) {
    const int groups = (Win + 3) >> 2;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= Hin * groups) return;
    const int iy = t / groups, ix0 = (t - iy * groups) * 4;
    const size_t nc = blockIdx.y;
    const float* src = tmp + nc * Hout * Win;
    const bool vec = vec_ok(tmp, Win) && vec_ok(dx, Win);
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    for (int e = yoff[iy]; e < yoff[iy + 1]; ++e) {
        const float* row = src + (size_t)yent[e].o * Win;
        const float w = yent[e].w;
        if (vec) {
            const float4 v = *reinterpret_cast<const float4*>(row + ix0);
            out[0] += v.x * w; out[1] += v.y * w; out[2] += v.z * w; out[3] += v.w * w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) out[k] += row[min(ix0 + k, Win - 1)] * w;
        }
    }
    store4(dx + (nc * Hin + iy) * Win, ix0, Win, out, vec);
}

// ---------------------------------------------------------------- decoder input assembly
// Interior index of padded index p (ReflectionPad2d(1)): p - 1, reflected at both ends.
__device__ __forceinline__ int refl1(int p, int n) {
    const int i = p - 1;
    return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
}

// out (N, C1+C2, H+2, W+2) = reflect_pad1(cat(up(x), skip)); x (N, C1, H/up, W/up), skip (N, C2, H, W) or none.  grid.y = n * Ctot + c.
__global__ __launch_bounds__(kBlock) void pad_cat_fwd_kernel(const float* __restrict__ x, int C1, int up, const float* __restrict__ skip,
                                                             int C2, float* __restrict__ out, int H, int W) {
    const int Hp = H + 2, Wp = W + 2, groups = (Wp + 3) >> 2;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= Hp * groups) return;
    const int p = t / groups, q0 = (t - p * groups) * 4;
    const int Ct = C1 + C2, n = blockIdx.y / Ct, c = blockIdx.y - n * Ct;
    const int r = refl1(p, H);
    const float* row;
    int u;
    if (c < C1) {
        const int h = H / up, w = W / up;
        row = x + (((size_t)n * C1 + c) * h + r / up) * w;
        u = up;
    } else {
        row = skip + (((size_t)n * C2 + (c - C1)) * H + r) * W;
        u = 1;
    }
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = row[refl1(min(q0 + k, Wp - 1), W) / u];
    store4(out + ((size_t)blockIdx.y * Hp + p) * Wp, q0, Wp, v, false);
}

// Padded indices that read interior index r (ascending): 0 if r == 1, r + 1, n + 1 if r == n - 2.
__device__ __forceinline__ int padded_of(int r, int n, int* ps) {
    int k = 0;
    if (r == 1) ps[k++] = 0;
    ps[k++] = r + 1;
    if (r == n - 2) ps[k++] = n + 1;
    return k;
}

// dx (N, C1, H/up, W/up) and dskip (N, C2, H, W) from dout (N, C1+C2, H+2, W+2): each output sums, in a fixed order (replica row, padded
// row, replica column, padded column), every padded position that copied it.  grid.y = n * Ctot + c.
__global__ __launch_bounds__(kBlock) void pad_cat_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dx, int C1, int up,
                                                             float* __restrict__ dskip, int C2, int H, int W) {
    const int Ct = C1 + C2, n = blockIdx.y / Ct, c = blockIdx.y - n * Ct;
    const int u = c < C1 ? up : 1, h = H / u, w = W / u, groups = (w + 3) >> 2;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= h * groups) return;
    const int iy = t / groups, ix0 = (t - iy * groups) * 4;
    const int Wp = W + 2;
    const float* g = dout + (size_t)blockIdx.y * (H + 2) * Wp;
    float* dst = c < C1 ? dx + (((size_t)n * C1 + c) * h + iy) * w : dskip + (((size_t)n * C2 + (c - C1)) * h + iy) * w;
    float* base = c < C1 ? dx : dskip;
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ix = min(ix0 + k, w - 1);
        float s = 0.f;
        for (int a = 0; a < u; ++a) {
            int ps[3];
            const int np = padded_of(u * iy + a, H, ps);
            for (int i = 0; i < np; ++i) {
                const float* gr = g + (size_t)ps[i] * Wp;
                for (int b = 0; b < u; ++b) {
                    int qs[3];
                    const int nq = padded_of(u * ix + b, W, qs);
                    for (int j = 0; j < nq; ++j) s += gr[qs[j]];
                }
            }
        }
        out[k] = s;
    }
    store4(dst, ix0, w, out, vec_ok(base, w));
}

// ---------------------------------------------------------------- crop + activation
// act 0: ELU(alpha = 1), act 1: sigmoid.
__device__ __forceinline__ float act_fwd(float v, int act) { return act == 0 ? (v > 0.f ? v : expm1f(v)) : 1.f / (1.f + expf(-v)); }
// from the saved output y (inplace-ELU semantics for ELU)
__device__ __forceinline__ float act_bwd(float g, float y, int act) { return act == 0 ? (y <= 0.f ? g * (y + 1.f) : g) : g * (y * (1.f - y)); }

// y (NC, H, W) = act(in[:, 1:-1, 1:-1]), in (NC, H+2, W+2).  grid.y = nc.
__global__ __launch_bounds__(kBlock) void crop_act_fwd_kernel(const float* __restrict__ in, float* __restrict__ y, int act, int H, int W) {
    const int groups = (W + 3) >> 2;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= H * groups) return;
    const int r = t / groups, x0 = (t - r * groups) * 4;
    const float* src = in + ((size_t)blockIdx.y * (H + 2) + r + 1) * (W + 2) + 1;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = act_fwd(src[min(x0 + k, W - 1)], act);
    store4(y + ((size_t)blockIdx.y * H + r) * W, x0, W, v, vec_ok(y, W));
}

// din (NC, H+2, W+2) = [interior: act'(y) * dy, ring: 0] -- every element written, the zero ring included.
__global__ __launch_bounds__(kBlock) void crop_act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                              float* __restrict__ din, int act, int H, int W) {
    const int Hp = H + 2, Wp = W + 2, groups = (Wp + 3) >> 2;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= Hp * groups) return;
    const int p = t / groups, q0 = (t - p * groups) * 4;
    const size_t off = ((size_t)blockIdx.y * H + (p - 1)) * W;
    const bool inner_row = p >= 1 && p <= H;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = q0 + k;
        v[k] = (inner_row && q >= 1 && q <= W) ? act_bwd(dy[off + q - 1], y[off + q - 1], act) : 0.f;
    }
    store4(din + ((size_t)blockIdx.y * Hp + p) * Wp, q0, Wp, v, false);
}

inline dim3 grid2(long long per_plane, long long planes) { return dim3((unsigned)((per_plane + kBlock - 1) / kBlock), (unsigned)planes); }

}  // namespace cd

using namespace cd;

extern "C" int cd_bicubic_fwd(const float* x, float* y, int NC, int Hin, int Win, int Hout, int Wout, const void* ytab,
                              const void* xtab, int norm, float sub, float div, void* stream) {
    if (!x || !y || !ytab || !xtab || NC <= 0 || NC > 65535 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return CD_ERR_INVALID_ARG;
    if (norm && div == 0.f) return CD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(bicubic_fwd_kernel, grid2((long long)Hout * ((Wout + 3) / 4), NC), dim3(kBlock), 0, (hipStream_t)stream, x, y,
                       Hin, Win, Hout, Wout, (const Tap4*)ytab, (const Tap4*)xtab, norm, sub, div);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

extern "C" int cd_bicubic_bwd(const float* dy, float* dx, float* tmp, int NC, int Hin, int Win, int Hout, int Wout, const int* yoff,
                              const void* yent, const int* xoff, const void* xent, void* stream) {
    if (!dy || !dx || !tmp || !yoff || !yent || !xoff || !xent || NC <= 0 || NC > 65535 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0)
        return CD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(bicubic_bwd_x_kernel, grid2((long long)Hout * ((Win + 3) / 4), NC), dim3(kBlock), 0, (hipStream_t)stream, dy, tmp,
                       Hout, Wout, Win, xoff, (const InvTap*)xent);
    CD_CHECK_LAUNCH();
    hipLaunchKernelGGL(bicubic_bwd_y_kernel, grid2((long long)Hin * ((Win + 3) / 4), NC), dim3(kBlock), 0, (hipStream_t)stream, tmp, dx,
                       Hout, Hin, Win, yoff, (const InvTap*)yent);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

static bool pad_cat_ok(int C1, int up, int C2, int N, int H, int W) {
    return C1 > 0 && C2 >= 0 && N > 0 && (up == 1 || up == 2) && H >= 2 && W >= 2 && H % up == 0 && W % up == 0 &&
           (long long)N * (C1 + C2) <= 65535;
}

extern "C" int cd_pad_cat_fwd(const float* x, int C1, int up, const float* skip, int C2, float* out, int N, int H, int W, void* stream) {
    if (!x || !out || !pad_cat_ok(C1, up, C2, N, H, W) || (C2 > 0) != (skip != nullptr)) return CD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(pad_cat_fwd_kernel, grid2((long long)(H + 2) * ((W + 5) / 4), (long long)N * (C1 + C2)), dim3(kBlock), 0,
                       (hipStream_t)stream, x, C1, up, skip, C2, out, H, W);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

extern "C" int cd_pad_cat_bwd(const float* dout, float* dx, int C1, int up, float* dskip, int C2, int N, int H, int W, void* stream) {
    if (!dout || !dx || !pad_cat_ok(C1, up, C2, N, H, W) || (C2 > 0) != (dskip != nullptr)) return CD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(pad_cat_bwd_kernel, grid2((long long)H * ((W + 3) / 4), (long long)N * (C1 + C2)), dim3(kBlock), 0,
                       (hipStream_t)stream, dout, dx, C1, up, dskip, C2, H, W);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

extern "C" int cd_crop_act_fwd(const float* in, float* y, int act, int NC, int H, int W, void* stream) {
    if (!in || !y || (act != 0 && act != 1) || NC <= 0 || NC > 65535 || H <= 0 || W <= 0) return CD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(crop_act_fwd_kernel, grid2((long long)H * ((W + 3) / 4), NC), dim3(kBlock), 0, (hipStream_t)stream, in, y, act, H, W);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

extern "C" int cd_crop_act_bwd(const float* dy, const float* y, float* din, int act, int NC, int H, int W, void* stream) {
    if (!dy || !y || !din || (act != 0 && act != 1) || NC <= 0 || NC > 65535 || H <= 0 || W <= 0) return CD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(crop_act_bwd_kernel, grid2((long long)(H + 2) * ((W + 5) / 4), NC), dim3(kBlock), 0, (hipStream_t)stream, dy, y,
                       din, act, H, W);
    CD_CHECK_LAUNCH();
    return CD_OK;
}
