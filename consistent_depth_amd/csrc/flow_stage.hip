// Flow-consistency masks for gfx950: the reference's mask stage (flow.py:199-228 -> utils/consistency.py) per pair batch
// (cd_flow_consistency_masks) and in the pair store's layout with valid-pixel counts (cd_flow_stage_masks).
// THIS FILE IS COMPILED WITH -ffp-contract=off (build_native.py EXTRA_FLAGS): the _rn intrinsics are plain operators in the
// toolchain's headers, and HIP's default -ffp-contract=fast fuses them in the backend -- (g + 1) * W - 1, the tap sums and
// sse += d * d became twelve fma per pixel, sums one rounding away from the reference's on some pixels, which a threshold placed ON a
// sum shows (tests/test_flow_stage_gpu.py, channel order).  A pragma does not reach the backend's fusion; the flag does.
#include "cd_common.h"

namespace cd {

// ---------------------------------------------------------------- flow-consistency masks
// Replaces /root/reference/utils/consistency.py:32-67 (called from flow.py:199-228): for direction k of a pair
//   inside_k = 0 <= x+u <= W-1 and 0 <= y+v <= H-1
//   mask_k   = inside_k  and  |flow_k - (-flow_{1-k} warped by flow_k)|^2 < flow_thresh^2
//                        and  sum_c (color_k - color_{1-k} warped by flow_k)^2 < C * color_thresh^2
// The warp is the reference's OTHER sampler (consistency.py:8-23): grid = 2*uv/(W,H) - 1 evaluated in fp64 and cast to
// fp32, then grid_sample(border, align_corners=False): ix = ((g+1)*W - 1)/2 clipped to [0, W-1] -- i.e. u - 0.5, not
// geometry.sample's u*W/(W-1) - 0.5.  Every rounding step of the reference is reproduced (explicit _rn intrinsics, no
// contraction), so the masks are bit-identical to the oracle.  One thread = one pixel of one direction; the four taps
// are shared by the flow and the colour test.
struct TapsB { int x0, y0, x1, y1; float wnw, wne, wsw, wse; bool in_x1, in_y1; };

__device__ __forceinline__ TapsB taps_border_grid(double idx_x, double idx_y, int W, int H) {
    const float gx = (float)__dsub_rn(__ddiv_rn(__dmul_rn(2.0, idx_x), (double)W), 1.0);
    const float gy = (float)__dsub_rn(__ddiv_rn(__dmul_rn(2.0, idx_y), (double)H), 1.0);
    float ix = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(gx, 1.f), (float)W), 1.f), 0.5f);
    float iy = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(gy, 1.f), (float)H), 1.f), 0.5f);
    ix = fminf(fmaxf(ix, 0.f), (float)(W - 1));
    iy = fminf(fmaxf(iy, 0.f), (float)(H - 1));
    const float x0f = floorf(ix), y0f = floorf(iy), x1f = __fadd_rn(x0f, 1.f), y1f = __fadd_rn(y0f, 1.f);
    TapsB t;
    t.x0 = (int)x0f; t.y0 = (int)y0f; t.x1 = t.x0 + 1; t.y1 = t.y0 + 1;
    t.in_x1 = t.x1 <= W - 1; t.in_y1 = t.y1 <= H - 1;
    t.wnw = __fmul_rn(__fsub_rn(x1f, ix), __fsub_rn(y1f, iy));
    t.wne = __fmul_rn(__fsub_rn(ix, x0f), __fsub_rn(y1f, iy));
    t.wsw = __fmul_rn(__fsub_rn(x1f, ix), __fsub_rn(iy, y0f));
    t.wse = __fmul_rn(__fsub_rn(ix, x0f), __fsub_rn(iy, y0f));
    return t;
}

// The four tap offsets of a pixel, shared by every channel sampled at that position.  Taps outside the image are CLAMPED to a
// valid address (and their product replaced by an exact 0 afterwards): every gather of a pixel is an unconditional load, so the
// 10 pair loads (2 flow + 3 colour channels x 2 rows: round 5, below) are all in flight before the first wait.  Round 1's version loaded the optional
// taps under their conditions -- a load under a divergent branch is followed by s_waitcnt vmcnt(0): twenty serialised round trips
// per pixel, 8 % of the HBM rate.
// Round 5: the two taps of a row are adjacent floats -- ONE 8-byte load at a 4-byte-aligned address (gfx950 global loads take it:
// hipcc emits global_load_dwordx2 for an align-4 pair) instead of two gathers: 10 gather instructions per pixel instead of 20 on a
// kernel bound by the texture-address path.  The pair starts at min(x0, W - 2): for x0 = W - 1 (only the clamped right border) the
// west tap is the pair's SECOND float and the east tap carries an exact 0.
struct TapIdx { int n, s; bool hi; };       // offsets of the two pairs; hi: x0 = W - 1
__device__ __forceinline__ TapIdx tap_offsets(const TapsB& t, int W) {
    const int xp = t.x0 < W - 2 ? t.x0 : W - 2, ys = t.in_y1 ? t.y1 : t.y0;
    return TapIdx{t.y0 * W + xp, ys * W + xp, t.x0 > W - 2};
}
struct TapVals { float nw, ne, sw, se; };
__device__ __forceinline__ TapVals tap_load(const float* __restrict__ src, const TapIdx& i) {
    const FloatPair n = *reinterpret_cast<const FloatPair*>(src + i.n), s = *reinterpret_cast<const FloatPair*>(src + i.s);
    return TapVals{i.hi ? n.b : n.a, n.b, i.hi ? s.b : s.a, s.b};
}
__device__ __forceinline__ float tap_sum(const TapVals& v, const TapsB& t) {
    // ((nw + ne) + sw) + se, each term rounded, taps outside the image contribute nothing
    float o = __fmul_rn(v.nw, t.wnw);
    o = __fadd_rn(o, t.in_x1 ? __fmul_rn(v.ne, t.wne) : 0.f);
    o = __fadd_rn(o, t.in_y1 ? __fmul_rn(v.sw, t.wsw) : 0.f);
    o = __fadd_rn(o, (t.in_x1 && t.in_y1) ? __fmul_rn(v.se, t.wse) : 0.f);
    return o;
}

constexpr int kMaskMaxC = 3;   // colour channels held in registers at once (RGB: one batch)

// The decision of ONE pixel p of ONE direction, from the loads to the comparison -- the only copy of the rounding sequence; both mask
// kernels below call it.  fl / fo: the (2,H,W) flow of this direction / of the opposite one; cr / ct: the (C,H,W) colours of the
// direction's own frame / of the frame its flow points into.  `rev`: the colour sum runs over the channels C-1 .. 0 instead of
// 0 .. C-1 (fp32 addition is not associative: (d0^2 + d1^2) + d2^2 and (d2^2 + d1^2) + d0^2 differ in the last bit on ~20 % of the
// pixels, and the reference sums the B,G,R order of its files while the resident colours are R,G,B).
__device__ __forceinline__ bool flow_consistent_pixel(const float* __restrict__ fl, const float* __restrict__ fo,
                                                      const float* __restrict__ cr, const float* __restrict__ ct, int C, bool rev,
                                                      float thr_flow, float thr_color, int H, int W, int p) {
    const int HW = H * W;
    const int y = p / W, x = p - y * W;
    const float u = fl[p], v = fl[HW + p];
    // channel summed at position c of the order (positions past C repeat a valid channel: loaded, never summed)
    auto chan = [&](int c) { return c < C ? (rev ? C - 1 - c : c) : (rev ? 0 : C - 1); };
    // the reference pixel's own colours do not depend on the flow: requested before the tap arithmetic (first kMaskMaxC channels)
    float own[kMaskMaxC];
#pragma unroll
    for (int c = 0; c < kMaskMaxC; ++c) own[c] = cr[(size_t)chan(c) * HW + p];
    const double idx_x = (double)u + (double)x, idx_y = (double)v + (double)y;
    const bool inside = idx_x >= 0.0 && idx_x <= (double)(W - 1) && idx_y >= 0.0 && idx_y <= (double)(H - 1);
    const TapsB t = taps_border_grid(idx_x, idx_y, W, H);
    const TapIdx ti = tap_offsets(t, W);
    const TapVals fu = tap_load(fo, ti), fv = tap_load(fo + HW, ti);
    TapVals cv[kMaskMaxC];
#pragma unroll
    for (int c = 0; c < kMaskMaxC; ++c) cv[c] = tap_load(ct + (size_t)chan(c) * HW, ti);
    // flow test: flow_k - (-(flow_{1-k} warped)) = flow_k + warped   (negation commutes exactly with the weighted sum)
    const float du = __fadd_rn(u, tap_sum(fu, t)), dv = __fadd_rn(v, tap_sum(fv, t));
    const float sse_f = __fadd_rn(__fmul_rn(du, du), __fmul_rn(dv, dv));
    float sse_c = 0.f;
#pragma unroll
    for (int c = 0; c < kMaskMaxC; ++c)
        if (c < C) {
            const float d = __fsub_rn(own[c], tap_sum(cv[c], t));
            sse_c = c == 0 ? __fmul_rn(d, d) : __fadd_rn(sse_c, __fmul_rn(d, d));
        }
    for (int c = kMaskMaxC; c < C; ++c) {   // (more than three colour channels: one at a time, same order of the sum)
        const float d = __fsub_rn(cr[(size_t)chan(c) * HW + p], tap_sum(tap_load(ct + (size_t)chan(c) * HW, ti), t));
        sse_c = __fadd_rn(sse_c, __fmul_rn(d, d));
    }
    return inside && sse_f < thr_flow && sse_c < thr_color;
}

__global__ __launch_bounds__(kBlock) void flow_consistency_mask_kernel(
    const float* __restrict__ flow_fwd, const float* __restrict__ flow_bwd, const float* __restrict__ color0,
    const float* __restrict__ color1, int C, float thr_flow, float thr_color, int H, int W, float* __restrict__ mask_fwd,
    float* __restrict__ mask_bwd) {
    const int HW = H * W, b = blockIdx.z, k = blockIdx.y;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= HW) return;
    const float* fl = (k == 0 ? flow_fwd : flow_bwd) + (size_t)b * 2 * HW;
    const float* fo = (k == 0 ? flow_bwd : flow_fwd) + (size_t)b * 2 * HW;
    const float* cr = (k == 0 ? color0 : color1) + (size_t)b * C * HW;
    const float* ct = (k == 0 ? color1 : color0) + (size_t)b * C * HW;
    const bool m = flow_consistent_pixel(fl, fo, cr, ct, C, false, thr_flow, thr_color, H, W, p);
    (k == 0 ? mask_fwd : mask_bwd)[(size_t)b * HW + p] = m ? 1.f : 0.f;
}

// The same masks in the pair store's layout (loaders/pair_store.py): flows (P,2,2,H,W) [pair, direction, (dx,dy)], the colours of
// the two frames found through pair_frames in the resident (F,C,H,W) array (no gathered copy), masks (P,2,1,H,W) as BYTES 0 / 1, and
// the number of valid pixels of every (pair, direction) -- what the reference's check_good_flow_pairs (flow.py:46-86) counts in the
// mask PNGs.  One workgroup = kBlock consecutive pixels of one direction of one pair.
//   bytes:  the four lanes whose bytes share an aligned 32-bit word of the output store it once (lane of the lowest address);
//           words cut by the ends of a plane (H*W % 4 != 0 moves the planes off the word grid) or of a wave are stored byte by
//           byte.  Every byte of a plane is written by exactly one lane, and nothing outside it.
//   counts: ballot + popcount per wave, LDS across the four waves, ONE integer atomic add per workgroup onto counts zeroed by
//           zero_counts_kernel earlier in the same call (integer adds: exact, independent of the order).
__global__ __launch_bounds__(kBlock) void zero_counts_kernel(int32_t* __restrict__ counts, int n) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) counts[i] = 0;
}

__global__ __launch_bounds__(kBlock) void flow_stage_mask_kernel(
    const float* __restrict__ flows, const float* __restrict__ color, const int64_t* __restrict__ pair_frames, int C, int rev,
    float thr_flow, float thr_color, int F, int H, int W, uint8_t* __restrict__ masks, int32_t* __restrict__ counts) {
    __shared__ int red[kBlock / kWave];
    const int HW = H * W, b = blockIdx.z, k = blockIdx.y;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const bool live = p < HW;
    const int pc = live ? p : HW - 1;       // no early exit: every lane takes part in the shuffles and the ballot below
    int64_t f_own = pair_frames[(size_t)b * 2 + k], f_tgt = pair_frames[(size_t)b * 2 + (1 - k)];
    f_own = f_own < 0 ? 0 : (f_own > F - 1 ? F - 1 : f_own);       // (validated by the host; never dereferenced out of range)
    f_tgt = f_tgt < 0 ? 0 : (f_tgt > F - 1 ? F - 1 : f_tgt);
    const float* fl = flows + ((size_t)b * 2 + k) * 2 * HW;
    const float* fo = flows + ((size_t)b * 2 + (1 - k)) * 2 * HW;
    const float* cr = color + (size_t)f_own * C * HW;
    const float* ct = color + (size_t)f_tgt * C * HW;
    const bool m = live && flow_consistent_pixel(fl, fo, cr, ct, C, rev != 0, thr_flow, thr_color, H, W, pc);

    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const size_t a = ((size_t)b * 2 + k) * HW + p;       // byte offset in `masks` (4-byte aligned base)
    const unsigned v = m ? 1u : 0u;
    const unsigned v1 = __shfl_down(v, 1, kWave), v2 = __shfl_down(v, 2, kWave), v3 = __shfl_down(v, 3, kWave);
    const int g = (int)(a & 3), first = lane - g;        // the word's lowest byte belongs to lane `first`, pixel p - g
    const bool whole = first >= 0 && first + 3 < kWave && p - g + 3 < HW;
    if (live) {
        if (!whole) masks[a] = (uint8_t)v;
        else if (g == 0) *reinterpret_cast<uint32_t*>(masks + a) = v | (v1 << 8) | (v2 << 16) | (v3 << 24);
    }
    const int n = (int)__popcll(__ballot(m));
    if (lane == 0) red[wid] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) s += red[w];
        atomicAdd(&counts[b * 2 + k], s);
    }
}

}  // namespace cd

extern "C" int cd_flow_consistency_masks(const float* flow_fwd, const float* flow_bwd, const float* color0, const float* color1,
                                         int C, double flow_thresh, double color_thresh, int B, int H, int W, float* mask_fwd,
                                         float* mask_bwd, void* stream) {
    if (!flow_fwd || !flow_bwd || !color0 || !color1 || !mask_fwd || !mask_bwd) return CD_ERR_INVALID_ARG;
    if (B <= 0 || B > 65535 || C <= 0 || H < 2 || W < 2 || !(flow_thresh > 0.0) || !(color_thresh > 0.0)) return CD_ERR_INVALID_ARG;
    // the reference compares fp32 sums with python floats under NumPy's weak-scalar rule: the thresholds are rounded to fp32
    const float thr_f = (float)(flow_thresh * flow_thresh), thr_c = (float)((double)C * (color_thresh * color_thresh));
    const int HW = H * W;
    hipLaunchKernelGGL(cd::flow_consistency_mask_kernel, dim3((HW + cd::kBlock - 1) / cd::kBlock, 2, B), dim3(cd::kBlock), 0,
                       (hipStream_t)stream, flow_fwd, flow_bwd, color0, color1, C, thr_f, thr_c, H, W, mask_fwd, mask_bwd);
    CD_CHECK_LAUNCH();
    return CD_OK;
}

extern "C" int cd_flow_stage_masks(const float* flows, const float* color, const int64_t* pair_frames, int C, int reverse_channels,
                                   double flow_thresh, double color_thresh, int P, int F, int H, int W, uint8_t* masks,
                                   int32_t* counts, void* stream) {
    if (!flows || !color || !pair_frames || !masks || !counts) return CD_ERR_INVALID_ARG;
    if (P <= 0 || P > 65535 || F <= 0 || C <= 0 || H < 2 || W < 2 || !(flow_thresh > 0.0) || !(color_thresh > 0.0)) return CD_ERR_INVALID_ARG;
    if (reverse_channels != 0 && reverse_channels != 1) return CD_ERR_INVALID_ARG;
    if ((uintptr_t)masks % 4 != 0 || (uintptr_t)counts % 4 != 0) return CD_ERR_INVALID_ARG;     // 32-bit stores / atomics
    if ((long long)H * W > 0x3fffffffLL) return CD_ERR_INVALID_ARG;                             // pixel offsets are ints
    const float thr_f = (float)(flow_thresh * flow_thresh), thr_c = (float)((double)C * (color_thresh * color_thresh));   // as above
    const int HW = H * W;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cd::zero_counts_kernel, dim3((2 * P + cd::kBlock - 1) / cd::kBlock), dim3(cd::kBlock), 0, s, counts, 2 * P);
    CD_CHECK_LAUNCH();
    hipLaunchKernelGGL(cd::flow_stage_mask_kernel, dim3((HW + cd::kBlock - 1) / cd::kBlock, 2, P), dim3(cd::kBlock), 0, s, flows, color,
                       pair_frames, C, reverse_channels, thr_f, thr_c, F, H, W, masks, counts);
    CD_CHECK_LAUNCH();
    return CD_OK;
}
