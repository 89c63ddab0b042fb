// ReflectionPad2d around the convolutions of the ResNet generator (reference models_pix2pix/networks.py:321-439): the
// memory-bound passes between two MFMA convolutions of a ResnetBlock, with the pad folded into them.
//   forward : gs_reflect_norm_apply  z = [res +] act(norm(y)) [* keep * keep_scale] written into a tensor padded by `pad` pixels,
//             interior and reflected border in ONE pass -- the next conv is a pad-0 conv on a dense tensor.  One thread per 16-byte
//             chunk (8 channels) of a PADDED pixel: it finds the pixel it mirrors (ReflectionPad2d excludes the edge: index -1 is
//             pixel 1, index H is pixel H-2), reads y / res / keep there and stores once.  A border chunk recomputes its source's
//             value (the line is in L2 from the interior thread) instead of waiting for it: no ordering between threads.
//             gs_reflect_pad_image: the fp32 NCHW input image padded in front of the first 7x7 conv.
//   backward: gs_reflect_fold_add    out = fold(dpad) [+ add]: every border element of the gradient w.r.t. the padded tensor is added
//             to the pixel it mirrors (a corner pixel's neighbour collects up to four images; at the smallest planes up to nine), in
//             ONE fixed order per output element (rows: own, low mirror, high mirror; columns likewise; then `add`), fp32 sums, one
//             16-bit rounding.  No atomics: two runs give equal bits.  `add` is the residual stream's gradient.
//             gs_reflect_fold_image: the same fold for the fp32 NCHW gradient of the padded input image.
//   head    : gs_tanh_fwd / gs_tanh_bwd, fp32 elementwise (t = tanh(x); d = gscale * dout * (1 - t) * (1 + t)).
#include "common.hpp"

namespace {

constexpr int RF_MAX_PAD = 8;

inline bool rf_al(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

inline int rf_grid(int64_t total) {
    int64_t b = cdiv64(total, 256);
    return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

// index of the pixel that padded index t (already shifted by -pad: -pad <= t < n + pad, pad < n) mirrors
__device__ __forceinline__ int rf_src(int t, int n) { return t < 0 ? -t : (t >= n ? 2 * (n - 1) - t : t); }

struct RfApplyArgs {
    const unsigned short* y;
    const float *a, *b;               // norm 1: scale / shift [C]; norm 2: mean / invstd [N][C]
    const unsigned short* res;        // interior of a tensor padded by rp
    const uint8_t* keep;
    unsigned short* z;
    float keep_scale;
    int norm, act, rp, p, H, W, C;
    int64_t total;                    // N * (H + 2p) * (W + 2p) * (C / 8)
};

template <int DT>
__global__ __launch_bounds__(256) void reflect_norm_apply_kernel(const RfApplyArgs a) {
    const int nch = a.C >> 3, PW = a.W + 2 * a.p, PH = a.H + 2 * a.p;
    const int RW = a.W + 2 * a.rp, RH = a.H + 2 * a.rp;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < a.total; idx += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(idx % nch) * 8;
        int64_t r = idx / nch;
        const int px = (int)(r % PW); r /= PW;
        const int py = (int)(r % PH);
        const int n = (int)(r / PH);
        const int sy = rf_src(py - a.p, a.H), sx = rf_src(px - a.p, a.W);
        const int64_t pix = ((int64_t)n * a.H + sy) * a.W + sx;
        float v[8];
        unpack8<DT>(*reinterpret_cast<const uint4*>(a.y + pix * a.C + c0), v);
        if (a.norm == 1) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = v[i] * a.a[c0 + i] + a.b[c0 + i];
        } else if (a.norm == 2) {
            const float* mu = a.a + (int64_t)n * a.C + c0;
            const float* is = a.b + (int64_t)n * a.C + c0;
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (v[i] - mu[i]) * is[i];
        }
        if (a.act == GS_ACT_RELU) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = v[i] > 0.f ? v[i] : 0.f;
        }
        if (a.keep) {
            const uint2 k = *reinterpret_cast<const uint2*>(a.keep + pix * a.C + c0);
            const unsigned int kw[2] = {k.x, k.y};
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] *= ((kw[i >> 2] >> (8 * (i & 3))) & 0xffu) ? a.keep_scale : 0.f;
        }
        if (a.res) {
            float rr[8];
            const int64_t rpix = ((int64_t)n * RH + sy + a.rp) * RW + sx + a.rp;
            unpack8<DT>(*reinterpret_cast<const uint4*>(a.res + rpix * a.C + c0), rr);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += rr[i];
        }
        const int64_t opix = ((int64_t)n * PH + py) * PW + px;
        *reinterpret_cast<uint4*>(a.z + opix * a.C + c0) = pack8<DT>(v);
    }
}

__global__ __launch_bounds__(256) void reflect_pad_image_kernel(const float* __restrict__ x, float* __restrict__ xp, int H, int W,
                                                                 int p, int64_t total) {
    const int PW = W + 2 * p, PH = H + 2 * p;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int px = (int)(idx % PW);
        int64_t r = idx / PW;
        const int py = (int)(r % PH);
        const int64_t plane = r / PH;
        xp[idx] = x[(plane * H + rf_src(py - p, H)) * W + rf_src(px - p, W)];
    }
}

// padded indices (rows or columns) whose gradient lands on pixel i of n: its own, the low mirror, the high mirror
__device__ __forceinline__ int rf_images(int i, int n, int p, int (&t)[3]) {
    int k = 0;
    t[k++] = i + p;
    if (i >= 1 && i <= p) t[k++] = p - i;
    if (i <= n - 2 && i >= n - 1 - p) t[k++] = p + 2 * (n - 1) - i;
    return k;
}

struct RfFoldArgs {
    const unsigned short *dpad, *add;
    unsigned short* out;
    int p, H, W, C;
    int64_t total;                    // N * H * W * (C / 8)
};

template <int DT>
__global__ __launch_bounds__(256) void reflect_fold_add_kernel(const RfFoldArgs a) {
    const int nch = a.C >> 3, PW = a.W + 2 * a.p, PH = a.H + 2 * a.p;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < a.total; idx += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(idx % nch) * 8;
        const int64_t pix = idx / nch;
        const int x = (int)(pix % a.W);
        const int64_t r = pix / a.W;
        const int y = (int)(r % a.H);
        const int n = (int)(r / a.H);
        int ty[3], tx[3];
        const int ny = rf_images(y, a.H, a.p, ty), nx = rf_images(x, a.W, a.p, tx);
        float s[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = 0.f;
        for (int iy = 0; iy < ny; ++iy)
            for (int ix = 0; ix < nx; ++ix) {
                float g[8];
                const int64_t q = ((int64_t)n * PH + ty[iy]) * PW + tx[ix];
                unpack8<DT>(*reinterpret_cast<const uint4*>(a.dpad + q * a.C + c0), g);
#pragma unroll
                for (int i = 0; i < 8; ++i) s[i] += g[i];
            }
        if (a.add) {
            float g[8];
            unpack8<DT>(*reinterpret_cast<const uint4*>(a.add + pix * a.C + c0), g);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] += g[i];
        }
        *reinterpret_cast<uint4*>(a.out + pix * a.C + c0) = pack8<DT>(s);
    }
}

__global__ __launch_bounds__(256) void reflect_fold_image_kernel(const float* __restrict__ dxp, float* __restrict__ dx, int H, int W,
                                                                  int p, int64_t total) {
    const int PW = W + 2 * p, PH = H + 2 * p;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int x = (int)(idx % W);
        int64_t r = idx / W;
        const int y = (int)(r % H);
        const int64_t plane = r / H;
        int ty[3], tx[3];
        const int ny = rf_images(y, H, p, ty), nx = rf_images(x, W, p, tx);
        float s = 0.f;
        for (int iy = 0; iy < ny; ++iy)
            for (int ix = 0; ix < nx; ++ix) s += dxp[(plane * PH + ty[iy]) * PW + tx[ix]];
        dx[idx] = s;
    }
}

__global__ __launch_bounds__(256) void tanh_fwd_kernel(const float* __restrict__ x, float* __restrict__ t, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) t[i] = tanhf(x[i]);
}

__global__ __launch_bounds__(256) void tanh_bwd_kernel(const float* __restrict__ t, const float* __restrict__ dout, float gscale,
                                                        float* __restrict__ d, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = t[i];
        d[i] = gscale * dout[i] * ((1.f - v) * (1.f + v));        // 1 - |v| is exact from 0.5 up: no cancellation where tanh saturates
    }
}

int rf_check(const char* who, int pad, int N, int H, int W, int C, int dtype) {
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "%s: bad dtype %d", who, dtype);
    GS_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "%s: N=%d H=%d W=%d C=%d (C must be a positive multiple of 8)", who, N,
                 H, W, C);
    GS_CHECK_ARG(pad >= 0 && pad <= RF_MAX_PAD, "%s: pad=%d out of 0..%d", who, pad, RF_MAX_PAD);
    GS_CHECK_ARG(H > pad && W > pad, "%s: Padding size should be less than the corresponding input dimension (pad %d, plane %d x %d)",
                 who, pad, H, W);
    return GS_OK;
}

int rf_check_image(const char* who, const float* a, const float* b, int pad, int N, int C, int H, int W) {
    GS_CHECK_ARG(a && b && rf_al(a, 4) && rf_al(b, 4), "%s: null or misaligned pointer", who);
    GS_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0, "%s: bad dims", who);
    GS_CHECK_ARG(pad >= 0 && pad <= RF_MAX_PAD, "%s: pad=%d out of 0..%d", who, pad, RF_MAX_PAD);
    GS_CHECK_ARG(H > pad && W > pad, "%s: Padding size should be less than the corresponding input dimension (pad %d, plane %d x %d)",
                 who, pad, H, W);
    return GS_OK;
}

}  // namespace

extern "C" int gs_reflect_norm_apply(const void* y, const float* coef_a, const float* coef_b, int norm, int act, const void* res,
                                     int res_pad, const uint8_t* keep_mask, float keep_scale, void* z, int pad, int N, int H, int W,
                                     int C, int dtype, void* stream) {
    int rc = rf_check("gs_reflect_norm_apply", pad, N, H, W, C, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(y && z && rf_al(y, 16) && rf_al(z, 16) && rf_al(res, 16) && rf_al(coef_a, 16) && rf_al(coef_b, 16),
                 "gs_reflect_norm_apply: null or misaligned pointer (16 bytes)");
    GS_CHECK_ARG(rf_al(keep_mask, 8), "gs_reflect_norm_apply: keep_mask must be 8-byte aligned");
    GS_CHECK_ARG(norm >= 0 && norm <= 2 && (norm == 0 ? (!coef_a && !coef_b) : (coef_a && coef_b)),
                 "gs_reflect_norm_apply: norm 0 takes no coefficients, 1 (scale / shift [C]) and 2 (mean / invstd [N][C]) need both");
    GS_CHECK_ARG(act == GS_ACT_NONE || act == GS_ACT_RELU, "gs_reflect_norm_apply: activation must be none or ReLU");
    GS_CHECK_ARG(res_pad >= 0 && res_pad <= RF_MAX_PAD, "gs_reflect_norm_apply: res_pad=%d out of 0..%d", res_pad, RF_MAX_PAD);
    GS_CHECK_ARG(z != y && z != res, "gs_reflect_norm_apply: z must not alias y or res");
    RfApplyArgs a{(const unsigned short*)y, coef_a, coef_b, (const unsigned short*)res, keep_mask, (unsigned short*)z, keep_scale,
                  norm, act, res_pad, pad, H, W, C, (int64_t)N * (H + 2 * pad) * (W + 2 * pad) * (C / 8)};
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GS_F16) reflect_norm_apply_kernel<GS_F16><<<rf_grid(a.total), 256, 0, s>>>(a);
    else reflect_norm_apply_kernel<GS_BF16><<<rf_grid(a.total), 256, 0, s>>>(a);
    GS_CHECK_LAUNCH("gs_reflect_norm_apply");
    return GS_OK;
}

extern "C" int gs_reflect_fold_add(const void* dpad, const void* add, void* out, int pad, int N, int H, int W, int C, int dtype,
                                   void* stream) {
    int rc = rf_check("gs_reflect_fold_add", pad, N, H, W, C, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(dpad && out && rf_al(dpad, 16) && rf_al(out, 16) && rf_al(add, 16),
                 "gs_reflect_fold_add: null or misaligned pointer (16 bytes)");
    GS_CHECK_ARG(out != dpad, "gs_reflect_fold_add: out must not alias dpad");
    RfFoldArgs a{(const unsigned short*)dpad, (const unsigned short*)add, (unsigned short*)out, pad, H, W, C,
                 (int64_t)N * H * W * (C / 8)};
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GS_F16) reflect_fold_add_kernel<GS_F16><<<rf_grid(a.total), 256, 0, s>>>(a);
    else reflect_fold_add_kernel<GS_BF16><<<rf_grid(a.total), 256, 0, s>>>(a);
    GS_CHECK_LAUNCH("gs_reflect_fold_add");
    return GS_OK;
}

extern "C" int gs_reflect_pad_image(const float* x, float* xp, int pad, int N, int C, int H, int W, void* stream) {
    int rc = rf_check_image("gs_reflect_pad_image", x, xp, pad, N, C, H, W);
    if (rc) return rc;
    GS_CHECK_ARG(x != xp, "gs_reflect_pad_image: xp must not alias x");
    const int64_t total = (int64_t)N * C * (H + 2 * pad) * (W + 2 * pad);
    reflect_pad_image_kernel<<<rf_grid(total), 256, 0, (hipStream_t)stream>>>(x, xp, H, W, pad, total);
    GS_CHECK_LAUNCH("gs_reflect_pad_image");
    return GS_OK;
}

extern "C" int gs_reflect_fold_image(const float* dxp, float* dx, int pad, int N, int C, int H, int W, void* stream) {
    int rc = rf_check_image("gs_reflect_fold_image", dxp, dx, pad, N, C, H, W);
    if (rc) return rc;
    GS_CHECK_ARG(dx != dxp, "gs_reflect_fold_image: dx must not alias dxp");
    const int64_t total = (int64_t)N * C * H * W;
    reflect_fold_image_kernel<<<rf_grid(total), 256, 0, (hipStream_t)stream>>>(dxp, dx, H, W, pad, total);
    GS_CHECK_LAUNCH("gs_reflect_fold_image");
    return GS_OK;
}

extern "C" int gs_tanh_fwd(const float* x, float* t, int64_t n, void* stream) {
    GS_CHECK_ARG(x && t && rf_al(x, 4) && rf_al(t, 4) && n > 0, "gs_tanh_fwd: null or misaligned pointer, or n < 1");
    tanh_fwd_kernel<<<rf_grid(n), 256, 0, (hipStream_t)stream>>>(x, t, n);
    GS_CHECK_LAUNCH("gs_tanh_fwd");
    return GS_OK;
}

extern "C" int gs_tanh_bwd(const float* t, const float* dout, float gscale, float* d, int64_t n, void* stream) {
    GS_CHECK_ARG(t && dout && d && rf_al(t, 4) && rf_al(dout, 4) && rf_al(d, 4) && n > 0,
                 "gs_tanh_bwd: null or misaligned pointer, or n < 1");
    tanh_bwd_kernel<<<rf_grid(n), 256, 0, (hipStream_t)stream>>>(t, dout, gscale, d, n);
    GS_CHECK_LAUNCH("gs_tanh_bwd");
    return GS_OK;
}
