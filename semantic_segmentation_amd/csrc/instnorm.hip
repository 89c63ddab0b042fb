// InstanceNorm2d(affine=False, track_running_stats=False) around the MFMA convolutions of the Pix2Pix networks under
// `--norm instance` (reference models_pix2pix/networks.py:23-38 get_norm_layer, :553-617 generator, :620-665 PatchGAN):
// statistics per (sample, channel) over the H*W plane of the stored 16-bit conv output, fused with the activation, the
// dropout keep mask and the concat write as gs_bn_act_apply / gs_bn_act_bwd_* are for BatchNorm.
//   forward : gs_in_stats -> gs_in_act_apply (one read of y, up to two outputs)
//   backward: gs_in_act_bwd = plane sums (+ their second stage) -> apply
// Work split of the two reductions (stats, backward sums): a block is 256 threads = PL pixel lanes x CL chunk lanes (a chunk =
// 8 channels = 16 bytes) of ONE sample; the grid is (chunk groups, S pixel slices of the plane, N).  Tiny planes take few pixel
// lanes and many chunks (2x2x512: PL 4 x CL 64, a block owns the 512 channels of one sample), large planes of few channels take
// 256 pixel lanes and S > 1 slices, whose partial results a second launch joins in slice order.  No atomics anywhere: every sum
// has one fixed order, so two runs give equal bits.
// Variance: each thread takes sums about ITS first pixel (fp32, a few dozen terms), turns them into (count, sum, M2) in double and
// the lanes / slices are joined with Chan's pairwise update in double -- centred at every level, nothing of the form E[y^2] - mean^2
// over a plane.  The plain sum travels instead of the mean: sums of 16-bit values are exact in double (fp16 always, bf16 over any
// range of 2^40), so mean = float(sum / HW) is the exact mean rounded, and an all-cancelling plane gives exactly zero.  The only
// fp32 roundings of mean and invstd are the final conversions.
#include "common.hpp"

namespace {

constexpr int IN_MAX_SLICES = 64;

struct InGeom {
    int nch, CL, PL, groups, S, pps;
};

// the same split for the statistics and the backward sums: a function of (N, H*W, C) alone
InGeom in_geom(int N, int HW, int C) {
    InGeom g;
    g.nch = C / 8;
    int plt = HW / 4;                                   // about four pixels per thread before a plane gets more lanes
    plt = plt < 1 ? 1 : (plt > 32 ? 32 : plt);
    int cl = 256 / plt;                                 // >= 8 chunk lanes: 128-byte runs per pixel
    g.CL = g.nch < cl ? g.nch : cl;
    g.PL = 256 / g.CL;
    g.groups = cdiv(g.nch, g.CL);
    int s_fill = 1024 / (N * g.groups);                 // slices until ~1024 blocks are in flight
    int s_work = cdiv(HW, g.PL * 8);                    // ... but at least eight pixels per thread
    int S = s_fill < s_work ? s_fill : s_work;
    S = S < 1 ? 1 : (S > IN_MAX_SLICES ? IN_MAX_SLICES : S);
    g.pps = cdiv(HW, S);
    g.S = cdiv(HW, g.pps);
    return g;
}

__device__ __forceinline__ float slope_of(int act) { return act == GS_ACT_RELU ? 0.f : (act == GS_ACT_LEAKY02 ? 0.2f : 1.f); }

// Chan's update of (na, sum a, M2 a) with (nb, sum b, M2 b); empty sides pass the other through
__device__ __forceinline__ void chan_join(int& na, double& sa, double& Ma, int nb, double sb, double Mb) {
    if (nb == 0) return;
    if (na == 0) { na = nb; sa = sb; Ma = Mb; return; }
    const double n = (double)(na + nb), d = sb / (double)nb - sa / (double)na;
    Ma += Mb + d * d * ((double)na * (double)nb / n);
    sa += sb;
    na += nb;
}

// ---- statistics ------------------------------------------------------------------------------------
// S == 1: writes mean / invstd.  S > 1: writes (sum, M2) of the slice to ws [N][S][2][C] (double); in_stats_join finishes.
template <int DT>
__global__ __launch_bounds__(256) void in_stats_kernel(const unsigned short* __restrict__ y, int HW, int C, InGeom g, double eps,
                                                       double* __restrict__ ws, float* __restrict__ mean, float* __restrict__ invstd) {
    __shared__ double sm[256][8], sM[256][8];
    __shared__ int sn[256];
    const int cl = threadIdx.x % g.CL, pl = threadIdx.x / g.CL;
    const int ch = blockIdx.x * g.CL + cl, s = blockIdx.y, n = blockIdx.z;
    const int p0 = s * g.pps, p1 = min(HW, p0 + g.pps);
    const bool lane_ok = pl < g.PL && ch < g.nch;
    int cnt = 0;
    double m[8], M2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { m[i] = 0.0; M2[i] = 0.0; }
    if (lane_ok && p0 + pl < p1) {
        const unsigned short* base = y + (int64_t)n * HW * C + ch * 8;
        float pv[8], s1[8], s2[8];
        unpack8<DT>(*reinterpret_cast<const uint4*>(base + (int64_t)(p0 + pl) * C), pv);
#pragma unroll
        for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
#pragma unroll 4
        for (int p = p0 + pl; p < p1; p += g.PL) {
            float v[8];
            unpack8<DT>(*reinterpret_cast<const uint4*>(base + (int64_t)p * C), v);
#pragma unroll
            for (int i = 0; i < 8; ++i) { const float d = v[i] - pv[i]; s1[i] += d; s2[i] += d * d; }
            ++cnt;
        }
        const double inv = 1.0 / (double)cnt;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double a = (double)s1[i], b = (double)s2[i];
            m[i] = (double)pv[i] * (double)cnt + a;          // the plain sum of the thread's pixels
            M2[i] = b - a * a * inv;
            if (M2[i] < 0.0) M2[i] = 0.0;
        }
    }
    // join the pixel lanes of a chunk lane: a fixed tree (lane pl takes lane pl + st)
    int top = 1;
    while (top < g.PL) top <<= 1;
    sn[threadIdx.x] = cnt;
#pragma unroll
    for (int i = 0; i < 8; ++i) { sm[threadIdx.x][i] = m[i]; sM[threadIdx.x][i] = M2[i]; }
    __syncthreads();
    for (int st = top >> 1; st >= 1; st >>= 1) {
        const bool take = pl < st && pl + st < g.PL;
        const int o = threadIdx.x + st * g.CL;
        if (take) {
            const int nb = sn[o];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                int na = cnt;
                chan_join(na, m[i], M2[i], nb, sm[o][i], sM[o][i]);
            }
            cnt += nb;
        }
        __syncthreads();
        if (take) {
            sn[threadIdx.x] = cnt;
#pragma unroll
            for (int i = 0; i < 8; ++i) { sm[threadIdx.x][i] = m[i]; sM[threadIdx.x][i] = M2[i]; }
        }
        __syncthreads();
    }
    if (pl != 0 || ch >= g.nch) return;
    if (g.S == 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double var = M2[i] / (double)HW;
            mean[(int64_t)n * C + ch * 8 + i] = (float)(m[i] / (double)HW);
            invstd[(int64_t)n * C + ch * 8 + i] = (float)(1.0 / sqrt(var + eps));
        }
    } else {
        double* o = ws + ((int64_t)n * g.S + s) * 2 * C + ch * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) { o[i] = m[i]; o[C + i] = M2[i]; }
    }
}

// one thread per (n, c): the slices in ascending order
__global__ __launch_bounds__(256) void in_stats_join(const double* __restrict__ ws, int NC, int C, int HW, int S, int pps, double eps,
                                                     float* __restrict__ mean, float* __restrict__ invstd) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= NC) return;
    const int n = t / C, c = t - n * C;
    int na = 0;
    double m = 0.0, M2 = 0.0;
    for (int s = 0; s < S; ++s) {
        const int nb = min(HW, (s + 1) * pps) - s * pps;
        const double* o = ws + ((int64_t)n * S + s) * 2 * C + c;
        chan_join(na, m, M2, nb, o[0], o[C]);
    }
    mean[t] = (float)(m / (double)HW);
    invstd[t] = (float)(1.0 / sqrt(M2 / (double)HW + eps));
}

// ---- forward apply ---------------------------------------------------------------------------------
struct InApplyArgs {
    const unsigned short* y;
    const float *mean, *invstd;
    unsigned short *z, *z2;
    const uint8_t* keep;
    float keep_scale;
    int act, zs, zc, act2, z2s, z2c;
    int HW, C;
    int64_t total;                // N * HW * (C / 8)
};

template <int DT>
__global__ __launch_bounds__(256) void in_act_apply_kernel(const InApplyArgs a) {
    const float sl = slope_of(a.act), sl2 = slope_of(a.act2);
    const int nch = a.C >> 3;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < a.total; idx += (int64_t)gridDim.x * 256) {
        const int ch = (int)(idx % nch);
        const int64_t pix = idx / nch;
        const int n = (int)(pix / a.HW);
        const int c0 = ch * 8;
        float v[8], mu[8], is[8], o[8];
        unpack8<DT>(*reinterpret_cast<const uint4*>(a.y + pix * a.C + c0), v);
        const float4* pm = reinterpret_cast<const float4*>(a.mean + (int64_t)n * a.C + c0);
        const float4* pi = reinterpret_cast<const float4*>(a.invstd + (int64_t)n * a.C + c0);
        const float4 m0 = pm[0], m1 = pm[1], i0 = pi[0], i1 = pi[1];
        mu[0] = m0.x; mu[1] = m0.y; mu[2] = m0.z; mu[3] = m0.w; mu[4] = m1.x; mu[5] = m1.y; mu[6] = m1.z; mu[7] = m1.w;
        is[0] = i0.x; is[1] = i0.y; is[2] = i0.z; is[3] = i0.w; is[4] = i1.x; is[5] = i1.y; is[6] = i1.z; is[7] = i1.w;
        float kf[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) kf[i] = 1.f;
        if (a.keep) {
            const uint2 k = *reinterpret_cast<const uint2*>(a.keep + pix * a.C + c0);
            const unsigned int kw[2] = {k.x, k.y};
#pragma unroll
            for (int i = 0; i < 8; ++i) kf[i] = ((kw[i >> 2] >> (8 * (i & 3))) & 0xffu) ? a.keep_scale : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[i] = (v[i] - mu[i]) * is[i];
            const float t = v[i] > 0.f ? v[i] : v[i] * sl;
            o[i] = a.keep ? t * kf[i] : t;
        }
        st16(a.z + pix * a.zs + a.zc + c0, pack8<DT>(o));
        if (a.z2) {
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = v[i] > 0.f ? v[i] : v[i] * sl2;
            st16(a.z2 + pix * a.z2s + a.z2c + c0, pack8<DT>(o));
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------
struct InBwdArgs {
    const unsigned short *y, *dza, *dzb;
    const uint8_t* keep;
    float keep_scale;
    const float *mean, *invstd;
    int sa, ca, act, act_b, HW, C;
};

// xh and g = act'(xh) * keep * dz_a + act_b'(xh) * dz_b of 8 channels at pixel `pix` of sample n (ReLU'(0) = 0, leaky'(0) = 0.2)
template <int DT>
__device__ __forceinline__ void in_g8(const InBwdArgs& a, int64_t pix, int c0, const float (&mu)[8], const float (&is)[8], float sl_a,
                                      float sl_b, float (&xh)[8], float (&g)[8]) {
    float v[8], da[8], db[8];
    unpack8<DT>(*reinterpret_cast<const uint4*>(a.y + pix * a.C + c0), v);
    unpack8<DT>(*reinterpret_cast<const uint4*>(a.dza + pix * a.sa + a.ca + c0), da);
    if (a.dzb) unpack8<DT>(*reinterpret_cast<const uint4*>(a.dzb + pix * a.C + c0), db);
    if (a.keep) {
        const uint2 k = *reinterpret_cast<const uint2*>(a.keep + pix * a.C + c0);
        const unsigned int kw[2] = {k.x, k.y};
#pragma unroll
        for (int i = 0; i < 8; ++i) da[i] *= ((kw[i >> 2] >> (8 * (i & 3))) & 0xffu) ? a.keep_scale : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        xh[i] = (v[i] - mu[i]) * is[i];
        const bool pos = xh[i] > 0.f;
        g[i] = da[i] * (pos ? 1.f : sl_a);
        if (a.dzb) g[i] += db[i] * (pos ? 1.f : sl_b);
    }
}

__device__ __forceinline__ void load8f(const float* p, float (&o)[8]) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

// plane sums s1 = sum g, s2 = sum g * xh (each term fp32, the sums double).  S == 1: writes the plane means gm [2][N][C];
// S > 1: the slice sums to ws [N][S][2][C] (double), in_bwd_join finishes.
template <int DT>
__global__ __launch_bounds__(256) void in_bwd_reduce_kernel(const InBwdArgs a, InGeom g, int N, double* __restrict__ ws,
                                                            float* __restrict__ gm) {
    __shared__ double r1[256][8], r2[256][8];
    const int cl = threadIdx.x % g.CL, pl = threadIdx.x / g.CL;
    const int ch = blockIdx.x * g.CL + cl, s = blockIdx.y, n = blockIdx.z;
    const int p0 = s * g.pps, p1 = min(a.HW, p0 + g.pps);
    const bool lane_ok = pl < g.PL && ch < g.nch;
    const float sl_a = slope_of(a.act), sl_b = slope_of(a.act_b);
    double s1[8], s2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { s1[i] = 0.0; s2[i] = 0.0; }
    if (lane_ok) {
        const int c0 = ch * 8;
        float mu[8], is[8];
        load8f(a.mean + (int64_t)n * a.C + c0, mu);
        load8f(a.invstd + (int64_t)n * a.C + c0, is);
#pragma unroll 2
        for (int p = p0 + pl; p < p1; p += g.PL) {
            float xh[8], gg[8];
            in_g8<DT>(a, (int64_t)n * a.HW + p, c0, mu, is, sl_a, sl_b, xh, gg);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float t = gg[i] * xh[i];
                s1[i] += (double)gg[i];
                s2[i] += (double)t;
            }
        }
    }
    int top = 1;
    while (top < g.PL) top <<= 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) { r1[threadIdx.x][i] = s1[i]; r2[threadIdx.x][i] = s2[i]; }
    __syncthreads();
    for (int st = top >> 1; st >= 1; st >>= 1) {
        const bool take = pl < st && pl + st < g.PL;
        const int o = threadIdx.x + st * g.CL;
        if (take) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { s1[i] += r1[o][i]; s2[i] += r2[o][i]; }
        }
        __syncthreads();
        if (take) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { r1[threadIdx.x][i] = s1[i]; r2[threadIdx.x][i] = s2[i]; }
        }
        __syncthreads();
    }
    if (pl != 0 || ch >= g.nch) return;
    if (g.S == 1) {
        const int64_t o = (int64_t)n * a.C + ch * 8, NC = (int64_t)N * a.C;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            gm[o + i] = (float)(s1[i] / (double)a.HW);
            gm[NC + o + i] = (float)(s2[i] / (double)a.HW);
        }
    } else {
        double* o = ws + ((int64_t)n * g.S + s) * 2 * a.C + ch * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) { o[i] = s1[i]; o[a.C + i] = s2[i]; }
    }
}

__global__ __launch_bounds__(256) void in_bwd_join(const double* __restrict__ ws, int NC, int C, int HW, int S, float* __restrict__ gm) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= NC) return;
    const int n = t / C, c = t - n * C;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < S; ++s) {
        const double* o = ws + ((int64_t)n * S + s) * 2 * C + c;
        s1 += o[0];
        s2 += o[C];
    }
    gm[t] = (float)(s1 / (double)HW);
    gm[(int64_t)NC + t] = (float)(s2 / (double)HW);
}

template <int DT>
__global__ __launch_bounds__(256) void in_bwd_apply_kernel(const InBwdArgs a, const float* __restrict__ gm, int64_t NC, int64_t total,
                                                           unsigned short* __restrict__ dy) {
    const float sl_a = slope_of(a.act), sl_b = slope_of(a.act_b);
    const int nch = a.C >> 3;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int ch = (int)(idx % nch);
        const int64_t pix = idx / nch;
        const int n = (int)(pix / a.HW);
        const int c0 = ch * 8;
        float mu[8], is[8], k1[8], k2[8], xh[8], g[8], o[8];
        load8f(a.mean + (int64_t)n * a.C + c0, mu);
        load8f(a.invstd + (int64_t)n * a.C + c0, is);
        load8f(gm + (int64_t)n * a.C + c0, k1);
        load8f(gm + NC + (int64_t)n * a.C + c0, k2);
        in_g8<DT>(a, pix, c0, mu, is, sl_a, sl_b, xh, g);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = is[i] * (g[i] - k1[i] - xh[i] * k2[i]);
        st16(dy + pix * a.C + c0, pack8<DT>(o));
    }
}

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

int in_check_shape(const char* who, int N, int H, int W, int C, int dtype) {
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "%s: bad dtype", who);
    GS_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "%s: N, H, W must be positive and C a positive multiple of 8", who);
    GS_CHECK_ARG((int64_t)H * W >= 2, "%s: Expected more than 1 spatial element per plane (H*W = %lld)", who, (long long)H * W);
    GS_CHECK_ARG((int64_t)N * H * W < 2147483647LL && (int64_t)H * W * C < 2147483647LL && (int64_t)N * C < 2147483647LL && N <= 65535,
                 "%s: tensor too large", who);
    return GS_OK;
}

int grid_for(int64_t total) {
    int64_t b = cdiv64(total, 256);
    return (int)(b > 256 * 16 ? 256 * 16 : b);
}

}  // namespace

extern "C" int64_t gs_in_ws_floats(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || (int64_t)H * W >= 2147483647LL) return 0;
    const InGeom g = in_geom(N, H * W, C);
    return g.S > 1 ? (int64_t)N * g.S * 2 * C * 2 : 0;        // doubles [N][S][2][C]
}

extern "C" int gs_in_stats(const void* y, float eps, float* mean, float* invstd, float* ws, int N, int H, int W, int C, int dtype,
                           void* stream) {
    int rc = in_check_shape("gs_in_stats", N, H, W, C, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(y && mean && invstd && al16(y) && al16(mean) && al16(invstd), "gs_in_stats: null or misaligned pointer (16 bytes)");
    GS_CHECK_ARG(eps >= 0.f, "gs_in_stats: eps must not be negative");
    const int HW = H * W;
    const InGeom g = in_geom(N, HW, C);
    GS_CHECK_ARG(g.S == 1 || (ws && al16(ws)), "gs_in_stats: this shape needs a 16-byte aligned workspace of gs_in_ws_floats floats");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(g.groups, g.S, N);
    if (dtype == GS_F16)
        in_stats_kernel<GS_F16><<<grid, 256, 0, s>>>((const unsigned short*)y, HW, C, g, (double)eps, (double*)ws, mean, invstd);
    else
        in_stats_kernel<GS_BF16><<<grid, 256, 0, s>>>((const unsigned short*)y, HW, C, g, (double)eps, (double*)ws, mean, invstd);
    if (g.S > 1) in_stats_join<<<cdiv(N * C, 256), 256, 0, s>>>((const double*)ws, N * C, C, HW, g.S, g.pps, (double)eps, mean, invstd);
    GS_CHECK_LAUNCH("gs_in_stats");
    return GS_OK;
}

static int in_act_ok(int act) { return act == GS_ACT_NONE || act == GS_ACT_RELU || act == GS_ACT_LEAKY02; }

extern "C" int gs_in_act_apply(const void* y, const float* mean, const float* invstd, int act, void* z, int z_pix_stride, int z_coff,
                               const uint8_t* keep_mask, float keep_scale, void* z2, int act2, int z2_pix_stride, int z2_coff, int N,
                               int H, int W, int C, int dtype, void* stream) {
    int rc = in_check_shape("gs_in_act_apply", N, H, W, C, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(y && mean && invstd && z && al16(y) && al16(mean) && al16(invstd) && al16(z) && al16(z2),
                 "gs_in_act_apply: null or misaligned pointer (16 bytes)");
    GS_CHECK_ARG((((uintptr_t)keep_mask) & 7) == 0, "gs_in_act_apply: keep_mask must be 8-byte aligned");
    GS_CHECK_ARG(in_act_ok(act) && (!z2 || in_act_ok(act2)), "gs_in_act_apply: activation must be none / ReLU / LeakyReLU(0.2)");
    GS_CHECK_ARG(z_coff >= 0 && z_pix_stride >= z_coff + C && z_pix_stride % 8 == 0 && z_coff % 8 == 0, "gs_in_act_apply: bad z stride");
    GS_CHECK_ARG(!z2 || (z2_coff >= 0 && z2_pix_stride >= z2_coff + C && z2_pix_stride % 8 == 0 && z2_coff % 8 == 0),
                 "gs_in_act_apply: bad z2 stride");
    InApplyArgs a{(const unsigned short*)y, mean, invstd, (unsigned short*)z, (unsigned short*)z2, keep_mask, keep_scale,
                  act, z_pix_stride, z_coff, act2, z2_pix_stride, z2_coff, H * W, C, (int64_t)N * H * W * (C / 8)};
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GS_F16) in_act_apply_kernel<GS_F16><<<grid_for(a.total), 256, 0, s>>>(a);
    else in_act_apply_kernel<GS_BF16><<<grid_for(a.total), 256, 0, s>>>(a);
    GS_CHECK_LAUNCH("gs_in_act_apply");
    return GS_OK;
}

extern "C" int gs_in_act_bwd(const void* y, const float* mean, const float* invstd, const void* dz_a, int sa, int coff_a, int act,
                             const uint8_t* keep_mask, float keep_scale, const void* dz_b, int act_b, void* dy, float* gmeans,
                             float* ws, int N, int H, int W, int C, int dtype, void* stream) {
    int rc = in_check_shape("gs_in_act_bwd", N, H, W, C, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(y && mean && invstd && dz_a && dy && gmeans && al16(y) && al16(mean) && al16(invstd) && al16(dz_a) && al16(dz_b) &&
                     al16(dy) && al16(gmeans),
                 "gs_in_act_bwd: null or misaligned pointer (16 bytes)");
    GS_CHECK_ARG((((uintptr_t)keep_mask) & 7) == 0, "gs_in_act_bwd: keep_mask must be 8-byte aligned");
    GS_CHECK_ARG(in_act_ok(act) && (!dz_b || in_act_ok(act_b)), "gs_in_act_bwd: activation must be none / ReLU / LeakyReLU(0.2)");
    GS_CHECK_ARG(coff_a >= 0 && sa >= coff_a + C && sa % 8 == 0 && coff_a % 8 == 0, "gs_in_act_bwd: bad dz_a stride");
    const int HW = H * W;
    const InGeom g = in_geom(N, HW, C);
    GS_CHECK_ARG(g.S == 1 || (ws && al16(ws)), "gs_in_act_bwd: this shape needs a 16-byte aligned workspace of gs_in_ws_floats floats");
    InBwdArgs a{(const unsigned short*)y, (const unsigned short*)dz_a, (const unsigned short*)dz_b, keep_mask, keep_scale, mean, invstd,
                sa, coff_a, act, act_b, HW, C};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(g.groups, g.S, N);
    const int64_t total = (int64_t)N * HW * (C / 8), NC = (int64_t)N * C;
    if (dtype == GS_F16) in_bwd_reduce_kernel<GS_F16><<<grid, 256, 0, s>>>(a, g, N, (double*)ws, gmeans);
    else in_bwd_reduce_kernel<GS_BF16><<<grid, 256, 0, s>>>(a, g, N, (double*)ws, gmeans);
    if (g.S > 1) in_bwd_join<<<cdiv(N * C, 256), 256, 0, s>>>((const double*)ws, N * C, C, HW, g.S, gmeans);
    if (dtype == GS_F16) in_bwd_apply_kernel<GS_F16><<<grid_for(total), 256, 0, s>>>(a, gmeans, NC, total, (unsigned short*)dy);
    else in_bwd_apply_kernel<GS_BF16><<<grid_for(total), 256, 0, s>>>(a, gmeans, NC, total, (unsigned short*)dy);
    GS_CHECK_LAUNCH("gs_in_act_bwd");
    return GS_OK;
}
