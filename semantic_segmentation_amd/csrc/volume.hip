// Volumes of any size in front of and behind UNet3D: what GenSeg-3D/transforms.py does to every item on the host (RandomFlip x3
// :33-44, NormalizeIntensity over the non-zero voxels :22-30, PadToDivisible :47-60, composed :69-76 / :90-94) and the three sums of
// the label Dice of GenSeg-3D/train_unet.py:46-47, as four entry points.  All of them are memory-bound element-wise / reduction
// kernels: 16-byte accesses on the aligned side, peeled heads and tails on the side whose rows start anywhere, 64-bit offsets.
//   gs_volume_nonzero_stats : fp64 {count, mean, std, 1 / (std + 1e-5)} per sample; per-wave shuffle -> per-block LDS -> one partial
//                             row per block in ws, a second small launch sums the rows in index order.  No atomics: bit-identical runs.
//   gs_volume_prepare       : flip + normalise + zero-pad (and the mask beside it) in ONE launch, statistics and flips read from
//                             device memory.
//   gs_volume_restore_labels: crop + un-flip of a uint8 label map.
//   gs_label_sums           : int64 {sum p t, sum p, sum t} per sample (exact, order-free) and the Dice over the batch in fp64.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int VS_MAX_BLOCKS = 128;   // partial rows per sample of the statistics
constexpr int LS_MAX_BLOCKS = 64;    // partial rows per sample of the label sums
constexpr int GRID_YZ_MAX = 65535;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
    return v;
}

// ---- statistics over the non-zero voxels ------------------------------------------------------------------------------------
// the IEEE compare: -0.0 is excluded and NaN is included, as `image != 0` does (transforms.py:26)
__device__ __forceinline__ void vs_acc(float v, double& c, double& s, double& q) {
    if (v != 0.0f) {
        const double d = (double)v;
        c += 1.0;
        s += d;
        q += d * d;
    }
}

__global__ __launch_bounds__(256) void volume_stats_partial_kernel(const float* __restrict__ x, int64_t per, double* __restrict__ ws) {
    __shared__ double red[4][3];
    const int n = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    const float* xs = x + (int64_t)n * per;
    // a sample starts at any element: peel to 16 bytes, float4 body, scalar tail (head and tail: block 0)
    int64_t head = (int64_t)((4 - (((uintptr_t)xs >> 2) & 3)) & 3);
    if (head > per) head = per;
    const int64_t nv = (per - head) >> 2;
    const int64_t tail0 = head + nv * 4;
    double c = 0.0, s = 0.0, q = 0.0;
    if (b == 0) {
        if (t < head) vs_acc(xs[t], c, s, q);
        const int64_t k = tail0 + (t - 64);
        if (t >= 64 && k < per) vs_acc(xs[k], c, s, q);
    }
    const float4* xv = reinterpret_cast<const float4*>(xs + head);
    const int64_t stride = (int64_t)gridDim.x * 256;
#pragma unroll 2
    for (int64_t i = (int64_t)b * 256 + t; i < nv; i += stride) {
        const float4 v = xv[i];
        vs_acc(v.x, c, s, q);
        vs_acc(v.y, c, s, q);
        vs_acc(v.z, c, s, q);
        vs_acc(v.w, c, s, q);
    }
    c = wave_sum_f64(c);
    s = wave_sum_f64(s);
    q = wave_sum_f64(q);
    if ((t & 63) == 0) {
        red[t >> 6][0] = c;
        red[t >> 6][1] = s;
        red[t >> 6][2] = q;
    }
    __syncthreads();
    if (t < 3) ws[((int64_t)n * VS_MAX_BLOCKS + b) * 3 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// rows summed in index order; var = (n Q - S^2) / (n (n - 1)) (unbiased, Tensor.std()), 1e-5 added to the std (transforms.py:29).
// count == 0: mean = 0 / 0 = NaN; count < 2: std = NaN, as torch gives for both -- the NaNs are kept and flow on.
__global__ __launch_bounds__(64) void volume_stats_finish_kernel(const double* __restrict__ ws, int N, int nb, double* __restrict__ stats) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const double* r = ws + (int64_t)n * VS_MAX_BLOCKS * 3;
    double c = 0.0, s = 0.0, q = 0.0;
    for (int b = 0; b < nb; ++b) {
        c += r[b * 3];
        s += r[b * 3 + 1];
        q += r[b * 3 + 2];
    }
    const double mean = s / c;
    double num = c * q - s * s;
    if (num < 0.0) num = 0.0;                       // rounding below zero on a constant sample; NaN stays NaN
    const double var = c > 1.0 ? num / (c * (c - 1.0)) : (double)NAN;
    const double sd = sqrt(var);
    stats[n * 4] = c;
    stats[n * 4 + 1] = mean;
    stats[n * 4 + 2] = sd;
    stats[n * 4 + 3] = 1.0 / (sd + 1e-5);
}

// ---- flip + normalise + pad ---------------------------------------------------------------------------------------------------
struct VolArgs {
    const float* x;
    const uint8_t* mask;
    const double* stats;
    const int32_t* flips;
    float* out;
    uint8_t* mask_out;
    int N, C, D, H, W, Dp, Hp, Wp;
};

// grid (x: blocks over one padded slice, y: padded depth, z: N*C image planes, then N mask planes).  A thread owns 16 bytes of the
// padded output (4 voxels of the image, 16 of the mask) and reads the source row dword by dword (bytes for the mask): the unpadded
// rows start at any element.  A W-flip reads the mirrored span and reverses it inside the vector.
__global__ __launch_bounds__(256) void volume_prepare_kernel(const VolArgs a) {
    const int d = blockIdx.y, z = blockIdx.z, NC = a.N * a.C;
    const int start = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    if (z < NC) {
        const int n = z / a.C;
        const int f = a.flips ? a.flips[n] : 0;
        const bool norm = a.stats != nullptr;
        const double mean = norm ? a.stats[n * 4 + 1] : 0.0, inv = norm ? a.stats[n * 4 + 3] : 1.0;
        const bool din = d < a.D;
        const int sd = din ? ((f & 1) ? a.D - 1 - d : d) : 0;
        const float* xslice = a.x + ((int64_t)z * a.D + sd) * ((int64_t)a.H * a.W);
        float* oslice = a.out + ((int64_t)z * a.Dp + d) * ((int64_t)a.Hp * a.Wp);
        const int wq = a.Wp >> 2, items = a.Hp * wq;
        for (int i = start; i < items; i += step) {
            const int h = i / wq, w0 = (i - h * wq) * 4;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (din && h < a.H && w0 < a.W) {
                const float* row = xslice + (int64_t)((f & 2) ? a.H - 1 - h : h) * a.W;
                const bool fw = (f & 4) != 0;
                const int sb = fw ? a.W - 4 - w0 : w0;          // source span [sb, sb + 4): mirrored under a W-flip
                float t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int sw = sb + j;
                    t[j] = (sw >= 0 && sw < a.W) ? row[sw] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xv = fw ? t[3 - j] : t[j];
                    if (w0 + j < a.W) v[j] = norm ? (float)(((double)xv - mean) * inv) : xv;
                }
            }
            *reinterpret_cast<float4*>(oslice + (int64_t)i * 4) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        const int n = z - NC;
        const int f = a.flips ? a.flips[n] : 0;
        const bool din = d < a.D;
        const int sd = din ? ((f & 1) ? a.D - 1 - d : d) : 0;
        const uint8_t* mslice = a.mask + ((int64_t)n * a.D + sd) * ((int64_t)a.H * a.W);
        uint8_t* oslice = a.mask_out + ((int64_t)n * a.Dp + d) * ((int64_t)a.Hp * a.Wp);
        const int w8 = a.Wp >> 3, items = (a.Hp * w8) >> 1;     // Hp is even: a 16-byte pair of 8-voxel groups stays in the slice
        const bool fw = (f & 4) != 0;
        for (int i = start; i < items; i += step) {
            unsigned int o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int grp = 2 * i + g, h = grp / w8, w0 = (grp - h * w8) * 8;
                if (din && h < a.H && w0 < a.W) {
                    const uint8_t* row = mslice + (int64_t)((f & 2) ? a.H - 1 - h : h) * a.W;
                    const int sb = fw ? a.W - 8 - w0 : w0;
                    unsigned int t[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int sw = sb + j;
                        t[j] = (sw >= 0 && sw < a.W) ? (unsigned int)row[sw] : 0u;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const unsigned int mv = fw ? t[7 - j] : t[j];
                        if (w0 + j < a.W) o[g * 2 + (j >> 2)] |= mv << (8 * (j & 3));
                    }
                }
            }
            *reinterpret_cast<uint4*>(oslice + (int64_t)i * 16) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

// ---- crop + un-flip of a label map -------------------------------------------------------------------------------------------
// grid (x: blocks over one output slice, y: output depth, z: sample).  A thread reads one aligned 8-byte group of a padded row and
// scatters its in-extent bytes to the (mirrored) positions of the unpadded row, which starts at any byte.
__global__ __launch_bounds__(256) void volume_restore_kernel(const uint8_t* __restrict__ lab, const int32_t* __restrict__ flips,
                                                             uint8_t* __restrict__ out, int D, int H, int W, int Dp, int Hp, int Wp) {
    const int d = blockIdx.y, n = blockIdx.z;
    const int f = flips ? flips[n] : 0;
    const int sd = (f & 1) ? D - 1 - d : d;
    const uint8_t* lslice = lab + ((int64_t)n * Dp + sd) * ((int64_t)Hp * Wp);
    uint8_t* oslice = out + ((int64_t)n * D + d) * ((int64_t)H * W);
    const int gw = (W + 7) >> 3, items = H * gw;
    const bool fw = (f & 4) != 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < items; i += gridDim.x * 256) {
        const int h = i / gw, w0 = (i - h * gw) * 8;
        const int sh = (f & 2) ? H - 1 - h : h;
        const uint2 v = *reinterpret_cast<const uint2*>(lslice + (int64_t)sh * Wp + w0);
        uint8_t* row = oslice + (int64_t)h * W;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sw = w0 + j;
            if (sw < W) row[fw ? W - 1 - sw : sw] = (uint8_t)(((j < 4 ? v.x : v.y) >> (8 * (j & 3))) & 0xffu);
        }
    }
}

// ---- the three sums of the label Dice ----------------------------------------------------------------------------------------
__device__ __forceinline__ void ls_acc(unsigned int p, unsigned int t, unsigned long long& I, unsigned long long& P,
                                       unsigned long long& T) {
    I += p * t;
    P += p;
    T += t;
}
// four bytes at once: sum p_i t_i, sum p_i, sum t_i of one dword pair (at most 4 * 255^2: no 32-bit sum lives longer than one vector)
__device__ __forceinline__ void ls_dword(unsigned int p, unsigned int t, unsigned int& i, unsigned int& sp, unsigned int& st) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned int pb = (p >> (8 * k)) & 0xffu, tb = (t >> (8 * k)) & 0xffu;
        i += pb * tb;
        sp += pb;
        st += tb;
    }
}

__global__ __launch_bounds__(256) void label_sums_partial_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ target,
                                                                 int64_t n_per, long long* __restrict__ ws) {
    __shared__ unsigned long long red[4][3];
    const int n = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    const uint8_t* ps = pred + (int64_t)n * n_per;
    const uint8_t* ts = target + (int64_t)n * n_per;
    // both maps share their offset inside 16 bytes (checked by the entry point): one peel serves both
    int64_t head = (int64_t)((16 - ((uintptr_t)ps & 15)) & 15);
    if (head > n_per) head = n_per;
    const int64_t nv = (n_per - head) >> 4;
    const int64_t tail0 = head + nv * 16;
    unsigned long long I = 0, P = 0, T = 0;
    if (b == 0) {
        if (t < head) ls_acc(ps[t], ts[t], I, P, T);
        const int64_t k = tail0 + (t - 64);
        if (t >= 64 && k < n_per) ls_acc(ps[k], ts[k], I, P, T);
    }
    const uint4* pv = reinterpret_cast<const uint4*>(ps + head);
    const uint4* tv = reinterpret_cast<const uint4*>(ts + head);
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)b * 256 + t; i < nv; i += stride) {
        const uint4 p4 = pv[i], t4 = tv[i];
        unsigned int vi = 0, vp = 0, vt = 0;                    // <= 16 * 255^2 per vector
        ls_dword(p4.x, t4.x, vi, vp, vt);
        ls_dword(p4.y, t4.y, vi, vp, vt);
        ls_dword(p4.z, t4.z, vi, vp, vt);
        ls_dword(p4.w, t4.w, vi, vp, vt);
        I += vi;
        P += vp;
        T += vt;
    }
    I = wave_sum_u64(I);
    P = wave_sum_u64(P);
    T = wave_sum_u64(T);
    if ((t & 63) == 0) {
        red[t >> 6][0] = I;
        red[t >> 6][1] = P;
        red[t >> 6][2] = T;
    }
    __syncthreads();
    if (t < 3) ws[((int64_t)n * LS_MAX_BLOCKS + b) * 3 + t] = (long long)(red[0][t] + red[1][t] + red[2][t] + red[3][t]);
}

// one block: per-sample rows summed, then (dice != NULL) the Dice over the batch, (2 I + eps) / (P + T + eps) in fp64 -> fp32
__global__ __launch_bounds__(64) void label_sums_finish_kernel(const long long* __restrict__ ws, int N, int nb, long long* sums,
                                                               float* __restrict__ dice, double eps) {
    for (int n = threadIdx.x; n < N; n += 64) {
        const long long* r = ws + (int64_t)n * LS_MAX_BLOCKS * 3;
        long long I = 0, P = 0, T = 0;
        for (int b = 0; b < nb; ++b) {
            I += r[b * 3];
            P += r[b * 3 + 1];
            T += r[b * 3 + 2];
        }
        sums[n * 3] = I;
        sums[n * 3 + 1] = P;
        sums[n * 3 + 2] = T;
    }
    if (dice == nullptr) return;
    __syncthreads();                                           // the block's own global stores are visible to it behind the barrier
    if (threadIdx.x == 0) {
        long long I = 0, P = 0, T = 0;
        for (int n = 0; n < N; ++n) {
            I += sums[n * 3];
            P += sums[n * 3 + 1];
            T += sums[n * 3 + 2];
        }
        dice[0] = (float)((2.0 * (double)I + eps) / ((double)P + (double)T + eps));
    }
}

bool volume_geometry_ok(const char* name, int N, int C, int D, int H, int W, int Dp, int Hp, int Wp) {
    if (!(N > 0 && C > 0 && D > 0 && H > 0 && W > 0)) {
        gs_set_error("%s: N=%d C=%d D=%d H=%d W=%d must all be positive", name, N, C, D, H, W);
        return false;
    }
    if (!(Dp >= D && Hp >= H && Wp >= W)) {
        gs_set_error("%s: padded dims %dx%dx%d are smaller than the volume %dx%dx%d", name, Dp, Hp, Wp, D, H, W);
        return false;
    }
    if ((Dp | Hp | Wp) & 7) {
        gs_set_error("%s: padded dims %dx%dx%d must be multiples of 8", name, Dp, Hp, Wp);
        return false;
    }
    if (!((int64_t)Hp * Wp < (1LL << 30) && Dp <= GRID_YZ_MAX && (int64_t)N * C + N <= GRID_YZ_MAX)) {
        gs_set_error("%s: volume too large (Hp*Wp < 2^30, Dp <= 65535, N*(C+1) <= 65535)", name);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int64_t gs_volume_stats_ws_doubles(int N) { return N > 0 ? (int64_t)N * VS_MAX_BLOCKS * 3 : 0; }

extern "C" int gs_volume_nonzero_stats(const float* x, int N, int64_t per_sample, double* ws, double* stats, void* stream) {
    GS_CHECK_ARG(x && ws && stats, "gs_volume_nonzero_stats: NULL pointer");
    GS_CHECK_ARG(N > 0 && N <= GRID_YZ_MAX && per_sample > 0 && per_sample < (1LL << 40),
                 "gs_volume_nonzero_stats: N=%d (1..65535) per_sample=%lld (1..2^40)", N, (long long)per_sample);
    GS_CHECK_ARG(((uintptr_t)x & 3) == 0 && (((uintptr_t)ws | (uintptr_t)stats) & 7) == 0,
                 "gs_volume_nonzero_stats: x must be 4-byte, ws / stats 8-byte aligned");
    int64_t nb = cdiv64(per_sample, 256 * 4 * 4);
    if (nb > VS_MAX_BLOCKS) nb = VS_MAX_BLOCKS;
    hipStream_t s = (hipStream_t)stream;
    volume_stats_partial_kernel<<<dim3((unsigned)nb, (unsigned)N), 256, 0, s>>>(x, per_sample, ws);
    volume_stats_finish_kernel<<<cdiv(N, 64), 64, 0, s>>>(ws, N, (int)nb, stats);
    GS_CHECK_LAUNCH("gs_volume_nonzero_stats");
    return GS_OK;
}

extern "C" int gs_volume_prepare(const float* x, const uint8_t* mask, const double* stats, const int32_t* flips, float* out,
                                 uint8_t* mask_out, int N, int C, int D, int H, int W, int Dp, int Hp, int Wp, void* stream) {
    GS_CHECK_ARG(x && out, "gs_volume_prepare: NULL pointer (x / out)");
    GS_CHECK_ARG((mask == nullptr) == (mask_out == nullptr), "gs_volume_prepare: mask / mask_out must both be given or NULL");
    if (!volume_geometry_ok("gs_volume_prepare", N, C, D, H, W, Dp, Hp, Wp)) return GS_EINVAL;
    GS_CHECK_ARG(((uintptr_t)x & 3) == 0 && (((uintptr_t)out | (uintptr_t)mask_out) & 15) == 0 && ((uintptr_t)stats & 7) == 0 &&
                     ((uintptr_t)flips & 3) == 0,
                 "gs_volume_prepare: out / mask_out must be 16-byte aligned (x, flips 4, stats 8)");
    const VolArgs a{x, mask, stats, flips, out, mask_out, N, C, D, H, W, Dp, Hp, Wp};
    int gx = cdiv(Hp * (Wp >> 2), 256);
    if (gx > 1024) gx = 1024;
    volume_prepare_kernel<<<dim3(gx, Dp, N * C + (mask ? N : 0)), 256, 0, (hipStream_t)stream>>>(a);
    GS_CHECK_LAUNCH("gs_volume_prepare");
    return GS_OK;
}

extern "C" int gs_volume_restore_labels(const uint8_t* lab, const int32_t* flips, uint8_t* out, int N, int D, int H, int W, int Dp,
                                        int Hp, int Wp, void* stream) {
    GS_CHECK_ARG(lab && out, "gs_volume_restore_labels: NULL pointer (lab / out)");
    if (!volume_geometry_ok("gs_volume_restore_labels", N, 1, D, H, W, Dp, Hp, Wp)) return GS_EINVAL;
    GS_CHECK_ARG(((uintptr_t)lab & 15) == 0 && ((uintptr_t)flips & 3) == 0,
                 "gs_volume_restore_labels: lab must be 16-byte aligned (flips 4)");
    int gx = cdiv(H * ((W + 7) >> 3), 256);
    if (gx > 1024) gx = 1024;
    volume_restore_kernel<<<dim3(gx, D, N), 256, 0, (hipStream_t)stream>>>(lab, flips, out, D, H, W, Dp, Hp, Wp);
    GS_CHECK_LAUNCH("gs_volume_restore_labels");
    return GS_OK;
}

extern "C" int64_t gs_label_sums_ws_int64(int N) { return N > 0 ? (int64_t)N * LS_MAX_BLOCKS * 3 : 0; }

extern "C" int gs_label_sums(const uint8_t* pred, const uint8_t* target, int N, int64_t n_per, int64_t* ws, int64_t* sums, float* dice,
                             double eps, void* stream) {
    GS_CHECK_ARG(pred && target && ws && sums, "gs_label_sums: NULL pointer");
    GS_CHECK_ARG(N > 0 && N <= GRID_YZ_MAX && n_per > 0 && n_per < (1LL << 40), "gs_label_sums: N=%d (1..65535) n_per=%lld (1..2^40)", N,
                 (long long)n_per);
    GS_CHECK_ARG((((uintptr_t)pred ^ (uintptr_t)target) & 15) == 0, "gs_label_sums: pred and target must share their offset within 16 bytes");
    GS_CHECK_ARG((((uintptr_t)ws | (uintptr_t)sums) & 7) == 0 && ((uintptr_t)dice & 3) == 0, "gs_label_sums: ws / sums 8-byte, dice 4-byte aligned");
    int64_t nb = cdiv64(n_per, 256 * 16 * 4);
    if (nb > LS_MAX_BLOCKS) nb = LS_MAX_BLOCKS;
    hipStream_t s = (hipStream_t)stream;
    label_sums_partial_kernel<<<dim3((unsigned)nb, (unsigned)N), 256, 0, s>>>(pred, target, n_per, (long long*)ws);
    label_sums_finish_kernel<<<1, 64, 0, s>>>((const long long*)ws, N, (int)nb, (long long*)sums, dice, eps);
    GS_CHECK_LAUNCH("gs_label_sums");
    return GS_OK;
}
