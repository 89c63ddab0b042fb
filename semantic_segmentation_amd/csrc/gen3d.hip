// Image-side tail of the 3-D Pix2Pix generator (GenSeg-3D/models/networks.py:688-692, the outermost block of the linear-upsample
// U-Net): Conv3d(C_in -> C_out, k 3, stride 1, pad 1) + bias + tanh from the dense 16-bit upsample output [N*D,H,W,C_in] to the fp32
// NCDHW image, C_in a multiple of 8 up to 64, C_out 1..4 -- below the generic engine's 8-channel granularity, and with a layout
// change and a tanh behind it.  27 C_in MACs per output and at most 4 outputs per voxel: bandwidth bound, so packed 16-bit loads and
// fp32 FMAs, no MFMA.
//   forward  a block owns an 8 x 32 tile of one depth slice and walks the three kz slices (and C_in in chunks of 32) through an LDS
//            halo tile [10][34][chunk]: every input voxel is fetched from memory about once (1.32x with the halo), not 27 times.  The
//            weights sit in LDS as [tap][ci][C_out] fp32 and are read wave-uniformly.
//   dx       the same tile over du = gscale * dout * (1 - t^2): the 3 x 10 x 34 halo of du (fp32, C_out planes) in LDS, a thread
//            takes its 27 C_out values into registers once and walks the C_in groups of 8 (weights [tap][co][ci]); fp32 sum, one
//            rounding.
//   dw, db   a block owns a run of voxels (a "part"); a thread owns the 8 input channels of one tap for every C_out and walks the
//            part (few items: several threads share an item and are added in a fixed order through LDS).  Per-part slabs go to the
//            workspace and a second launch adds them in a fixed order (eight interleaved runs of parts, then those): no atomics, two runs
//            give equal bits.
#include "common.hpp"

namespace {

constexpr int G3_TH = 8, G3_TW = 32;                  // output tile of one depth slice: one voxel per thread
constexpr int G3_HH = G3_TH + 2, G3_HW = G3_TW + 2;   // its halo
constexpr int G3_CC = 32;                             // input channels per LDS chunk of the forward
constexpr int G3_PS = G3_CC / 8 + 1;                  // halo pixel stride in 16-byte units (+1: lanes of a row spread over the banks)
constexpr int G3_CMAX = 64, G3_COMAX = 4;
constexpr int G3_VPP = 256;                           // voxels per part of the weight gradient (until G3_PMAX parts are reached)
constexpr int G3_PMAX = 1024;

struct G3Args {
    const unsigned short* x;      // [N*D,H,W,Cin]
    const float* w;               // [Cout][Cin][3][3][3]
    const float* bias;            // [Cout] or null
    float* out;                   // forward: [N,Cout,D,H,W]
    const float* t;               // backward: the forward's output (act tanh) or null
    const float* dout;            // backward: [N,Cout,D,H,W]
    unsigned short* dx;           // backward: [N*D,H,W,Cin] or null
    float* ws;
    int N, D, H, W, Cin, tiles_x, tiles_y, act;
    float gscale;
};

__device__ __forceinline__ void g3_tile(const G3Args& a, int& n, int& z, int& y0, int& x0) {
    int b = blockIdx.x;
    x0 = (b % a.tiles_x) * G3_TW; b /= a.tiles_x;
    y0 = (b % a.tiles_y) * G3_TH; b /= a.tiles_y;
    z = b % a.D;
    n = b / a.D;
}

template <int DT, int CO>
__global__ __launch_bounds__(256) void g3_tail_fwd_kernel(G3Args a) {
    __shared__ float wl[27 * G3_CMAX * CO];
    __shared__ uint4 halo[G3_HH * G3_HW * G3_PS];
    const int tid = threadIdx.x, Cin = a.Cin;
    int n, z, y0, x0;
    g3_tile(a, n, z, y0, x0);
    for (int i = tid; i < 27 * Cin * CO; i += 256) {
        const int co = i % CO, r = i / CO, ci = r % Cin, tap = r / Cin;
        wl[i] = a.w[((int64_t)co * Cin + ci) * 27 + tap];
    }
    const int ly = tid >> 5, lx = tid & 31;
    float acc[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) acc[co] = 0.f;
    for (int kz = 0; kz < 3; ++kz) {
        const int zz = z + kz - 1;
        if ((unsigned)zz >= (unsigned)a.D) continue;             // block-uniform: depth taps never leave the sample
        for (int c0 = 0; c0 < Cin; c0 += G3_CC) {
            const int ng = (Cin - c0 < G3_CC ? Cin - c0 : G3_CC) >> 3;
            __syncthreads();                                     // the previous chunk is consumed (and wl is written)
            for (int i = tid; i < G3_HH * G3_HW * ng; i += 256) {
                const int g = i % ng, p = i / ng, hx = p % G3_HW, hy = p / G3_HW;
                const int y = y0 + hy - 1, x = x0 + hx - 1;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W)
                    v = *reinterpret_cast<const uint4*>(a.x + ((((int64_t)n * a.D + zz) * a.H + y) * a.W + x) * Cin + c0 + g * 8);
                halo[p * G3_PS + g] = v;
            }
            __syncthreads();
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const uint4* hp = halo + ((ly + ky) * G3_HW + lx + kx) * G3_PS;
                    const float* wp = wl + ((kz * 9 + ky * 3 + kx) * Cin + c0) * CO;
                    for (int g = 0; g < ng; ++g) {
                        float f[8];
                        unpack8<DT>(hp[g], f);
#pragma unroll
                        for (int i = 0; i < 8; ++i)
#pragma unroll
                            for (int co = 0; co < CO; ++co) acc[co] += f[i] * wp[(g * 8 + i) * CO + co];
                    }
                }
        }
    }
    const int y = y0 + ly, x = x0 + lx;
    if (y < a.H && x < a.W) {
#pragma unroll
        for (int co = 0; co < CO; ++co) {
            float v = acc[co] + (a.bias ? a.bias[co] : 0.f);
            if (a.act == GS_ACT_TANH) v = tanhf(v);
            a.out[((((int64_t)n * CO + co) * a.D + z) * a.H + y) * a.W + x] = v;
        }
    }
}

// du of one voxel and channel: gscale * dout * (1 - t^2) (t null: act none)
__device__ __forceinline__ float g3_du(const G3Args& a, int64_t idx) {
    float d = a.gscale * a.dout[idx];
    if (a.t) {
        const float t = a.t[idx];
        d *= 1.f - t * t;
    }
    return d;
}

template <int DT, int CO>
__global__ __launch_bounds__(256) void g3_tail_dx_kernel(G3Args a) {
    __shared__ float wl[27 * CO * G3_CMAX];                      // [tap][co][ci]
    __shared__ float dh[3 * CO * G3_HH * G3_HW];                 // [slice z-1..z+1][co][halo row][halo column]
    const int tid = threadIdx.x, Cin = a.Cin;
    int n, z, y0, x0;
    g3_tile(a, n, z, y0, x0);
    for (int i = tid; i < 27 * CO * Cin; i += 256) {
        const int ci = i % Cin, r = i / Cin, co = r % CO, tap = r / CO;
        wl[i] = a.w[((int64_t)co * Cin + ci) * 27 + tap];
    }
    for (int i = tid; i < 3 * CO * G3_HH * G3_HW; i += 256) {
        const int hx = i % G3_HW;
        int r = i / G3_HW;
        const int hy = r % G3_HH; r /= G3_HH;
        const int co = r % CO, s = r / CO;
        const int zz = z - 1 + s, y = y0 - 1 + hy, x = x0 - 1 + hx;
        float d = 0.f;
        if ((unsigned)zz < (unsigned)a.D && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W)
            d = g3_du(a, ((((int64_t)n * CO + co) * a.D + zz) * a.H + y) * a.W + x);
        dh[i] = d;
    }
    __syncthreads();
    const int ly = tid >> 5, lx = tid & 31;
    // dx[z,y,x] = sum over taps of du[z+1-kz, y+1-ky, x+1-kx] * w[kz,ky,kx]: halo entry (2-kz, ly+2-ky, lx+2-kx)
    float dv[27 * CO];
#pragma unroll
    for (int kz = 0; kz < 3; ++kz)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int co = 0; co < CO; ++co)
                    dv[((kz * 3 + ky) * 3 + kx) * CO + co] = dh[(((2 - kz) * CO + co) * G3_HH + ly + 2 - ky) * G3_HW + lx + 2 - kx];
    const int y = y0 + ly, x = x0 + lx;
    if (y >= a.H || x >= a.W) return;
    unsigned short* const dst = a.dx + ((((int64_t)n * a.D + z) * a.H + y) * a.W + x) * Cin;
    for (int g = 0; g < (Cin >> 3); ++g) {
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
        for (int tc = 0; tc < 27 * CO; ++tc) {
            const float4 w0 = *reinterpret_cast<const float4*>(wl + tc * Cin + g * 8);
            const float4 w1 = *reinterpret_cast<const float4*>(wl + tc * Cin + g * 8 + 4);
            const float d = dv[tc];
            acc[0] += d * w0.x; acc[1] += d * w0.y; acc[2] += d * w0.z; acc[3] += d * w0.w;
            acc[4] += d * w1.x; acc[5] += d * w1.y; acc[6] += d * w1.z; acc[7] += d * w1.w;
        }
        st16(dst + g * 8, pack8<DT>(acc));
    }
}

// slab of part p: [Cout][Cin][27] then [Cout] (the bias gradient)
template <int DT, int CO>
__global__ __launch_bounds__(256) void g3_tail_dw_kernel(G3Args a, int nvox, int vpp, int ipb) {     // (nvox < 2^29: 32-bit voxel indices)
    __shared__ float red[256 * 8 * CO];
    const int Cin = a.Cin, G = Cin >> 3, items = 27 * G, T = CO * Cin * 27;
    const int il = threadIdx.x % ipb, sub = threadIdx.x / ipb, sub_n = 256 / ipb;
    const bool live = il < items;
    const int g = live ? il % G : 0, tap = live ? il / G : 0;
    const int kz = tap / 9 - 1, ky = (tap / 3) % 3 - 1, kx = tap % 3 - 1;
    const int v0 = blockIdx.x * vpp, v1 = v0 + vpp < nvox ? v0 + vpp : nvox;
    const int plane = a.D * a.H * a.W;
    float acc[CO][8];
#pragma unroll
    for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[co][i] = 0.f;
    if (live)
        for (int v = v0 + sub; v < v1; v += sub_n) {
            const int x = v % a.W;
            int r = v / a.W;
            const int y = r % a.H; r /= a.H;
            const int z = r % a.D;
            const int n = r / a.D;
            const int zz = z + kz, yy = y + ky, xx = x + kx;
            if ((unsigned)zz >= (unsigned)a.D || (unsigned)yy >= (unsigned)a.H || (unsigned)xx >= (unsigned)a.W) continue;
            const int sp = v - n * plane;                        // the voxel inside its sample
            float d[CO];
            bool any = false;
#pragma unroll
            for (int co = 0; co < CO; ++co) {
                d[co] = g3_du(a, ((int64_t)n * CO + co) * plane + sp);
                any |= d[co] != 0.f;
            }
            if (!any) continue;
            float f[8];
            unpack8<DT>(*reinterpret_cast<const uint4*>(a.x + ((((int64_t)n * a.D + zz) * a.H + yy) * a.W + xx) * Cin + g * 8), f);
#pragma unroll
            for (int co = 0; co < CO; ++co)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[co][i] += d[co] * f[i];
        }
    if (sub_n > 1) {
#pragma unroll
        for (int co = 0; co < CO; ++co)
#pragma unroll
            for (int i = 0; i < 8; ++i) red[(threadIdx.x * CO + co) * 8 + i] = acc[co][i];
        __syncthreads();
        if (sub == 0)
            for (int s = 1; s < sub_n; ++s)
#pragma unroll
                for (int co = 0; co < CO; ++co)
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[co][i] += red[((s * ipb + il) * CO + co) * 8 + i];
    }
    float* const slab = a.ws + (int64_t)blockIdx.x * (T + CO);
    if (sub == 0 && live) {
#pragma unroll
        for (int co = 0; co < CO; ++co)
#pragma unroll
            for (int i = 0; i < 8; ++i) slab[((int64_t)co * Cin + g * 8 + i) * 27 + tap] = acc[co][i];
    }
    if (threadIdx.x < 64) {                                      // the part's share of db: one wave, fixed order
#pragma unroll
        for (int co = 0; co < CO; ++co) {
            float s = 0.f;
            for (int v = v0 + (int)threadIdx.x; v < v1; v += 64) {
                const int n = v / plane;
                s += g3_du(a, ((int64_t)n * CO + co) * plane + (v - n * plane));
            }
            s = wave_sum(s);
            if (threadIdx.x == 0) slab[T + co] = s;
        }
    }
}

// dw[i] = sum over the parts (the last Cout elements of a slab are db): thread (pl, io) adds the parts pl, pl + 8, ... of element
// i0 + io in order, the eight partial sums are added in order through LDS -- a fixed order, two runs give equal bits
__global__ __launch_bounds__(256) void g3_tail_reduce_kernel(const float* ws, int nparts, int T, int CO, float* dw, float* db) {
    __shared__ float red[256];
    const int io = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + io;
    float s = 0.f;
    if (i < T + CO)
        for (int p = pl; p < nparts; p += 8) s += ws[(int64_t)p * (T + CO) + i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (pl == 0 && i < T + CO) {
        for (int k = 1; k < 8; ++k) s += red[k * 32 + io];
        if (i < T) dw[i] = s;
        else db[i - T] = s;
    }
}

int g3_parts(int64_t nvox) {
    const int64_t p = cdiv64(nvox, G3_VPP);
    return (int)(p < 1 ? 1 : p > G3_PMAX ? G3_PMAX : p);
}

int g3_check(const char* who, const void* x16, const float* w, int N, int D, int H, int W, int Cin, int Cout, int act, int dtype) {
    GS_CHECK_ARG(w && ((uintptr_t)w & 3) == 0, "%s: null or misaligned weight", who);
    GS_CHECK_ARG(((uintptr_t)x16 & 15) == 0, "%s: the 16-bit tensors must be 16-byte aligned", who);
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "%s: bad dtype", who);
    GS_CHECK_ARG(N > 0 && D > 0 && H > 0 && W > 0, "%s: bad dims", who);
    if (Cin < 8 || Cin > G3_CMAX || Cin % 8 != 0 || Cout < 1 || Cout > G3_COMAX || (act != GS_ACT_NONE && act != GS_ACT_TANH)) {
        gs_set_error("%s: C_in must be a multiple of 8 up to %d, C_out 1..%d, act none or tanh; got C_in=%d, C_out=%d, act=%d", who,
                     G3_CMAX, G3_COMAX, Cin, Cout, act);
        return GS_EUNSUPPORTED;
    }
    GS_CHECK_ARG((int64_t)N * D * H * W < 2147483647LL / 4, "%s: too many voxels", who);
    GS_CHECK_ARG((int64_t)N * D * cdiv(H, G3_TH) * cdiv(W, G3_TW) < 2147483647LL, "%s: too many tiles", who);
    return GS_OK;
}

}  // namespace

#define G3_DISPATCH(KERNEL, grid, ...)                                             \
    do {                                                                           \
        if (dtype == GS_F16) {                                                     \
            if (Cout == 1) KERNEL<GS_F16, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);    \
            else if (Cout == 2) KERNEL<GS_F16, 2><<<grid, 256, 0, s>>>(__VA_ARGS__); \
            else if (Cout == 3) KERNEL<GS_F16, 3><<<grid, 256, 0, s>>>(__VA_ARGS__); \
            else KERNEL<GS_F16, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);              \
        } else {                                                                   \
            if (Cout == 1) KERNEL<GS_BF16, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);   \
            else if (Cout == 2) KERNEL<GS_BF16, 2><<<grid, 256, 0, s>>>(__VA_ARGS__); \
            else if (Cout == 3) KERNEL<GS_BF16, 3><<<grid, 256, 0, s>>>(__VA_ARGS__); \
            else KERNEL<GS_BF16, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);             \
        }                                                                          \
    } while (0)

extern "C" int gs_conv3d_tail_fwd(const void* x, const float* w, const float* bias, float* out, int N, int D, int H, int W, int Cin,
                                  int Cout, int act, int dtype, void* stream) {
    int rc = g3_check("gs_conv3d_tail_fwd", x, w, N, D, H, W, Cin, Cout, act, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(x && out && (((uintptr_t)out | (uintptr_t)bias) & 3) == 0, "gs_conv3d_tail_fwd: null or misaligned x / out / bias");
    const int tiles_x = cdiv(W, G3_TW), tiles_y = cdiv(H, G3_TH);
    G3Args a{(const unsigned short*)x, w, bias, out, nullptr, nullptr, nullptr, nullptr, N, D, H, W, Cin, tiles_x, tiles_y, act, 1.f};
    hipStream_t s = (hipStream_t)stream;
    const int nb = N * D * tiles_y * tiles_x;
    G3_DISPATCH(g3_tail_fwd_kernel, nb, a);
    GS_CHECK_LAUNCH("gs_conv3d_tail_fwd");
    return GS_OK;
}

extern "C" int64_t gs_conv3d_tail_bwd_ws_floats(int N, int D, int H, int W, int Cin, int Cout) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
    return (int64_t)g3_parts((int64_t)N * D * H * W) * ((int64_t)Cout * Cin * 27 + Cout);
}

extern "C" int gs_conv3d_tail_bwd(const void* x, const float* w, const float* t, const float* dout, void* dx, float* dw, float* db,
                                  float* ws, int N, int D, int H, int W, int Cin, int Cout, int act, float gscale, int dtype,
                                  void* stream) {
    int rc = g3_check("gs_conv3d_tail_bwd", x, w, N, D, H, W, Cin, Cout, act, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(dout && (((uintptr_t)dout | (uintptr_t)t) & 3) == 0, "gs_conv3d_tail_bwd: null or misaligned dout / t");
    GS_CHECK_ARG(act != GS_ACT_TANH || t, "gs_conv3d_tail_bwd: act tanh needs the forward's output t");
    GS_CHECK_ARG(((uintptr_t)dx & 15) == 0, "gs_conv3d_tail_bwd: dx must be 16-byte aligned");
    GS_CHECK_ARG((dw == nullptr) == (db == nullptr) && (((uintptr_t)dw | (uintptr_t)db) & 3) == 0,
                 "gs_conv3d_tail_bwd: dw and db go together, 4-byte aligned");
    GS_CHECK_ARG(dw == nullptr || (x && ws && ((uintptr_t)ws & 3) == 0), "gs_conv3d_tail_bwd: the weight gradient needs x and a workspace");
    GS_CHECK_ARG(dx || dw, "gs_conv3d_tail_bwd: nothing to compute");
    const int tiles_x = cdiv(W, G3_TW), tiles_y = cdiv(H, G3_TH);
    G3Args a{(const unsigned short*)x, w, nullptr, nullptr, act == GS_ACT_TANH ? t : nullptr, dout, (unsigned short*)dx, ws,
             N, D, H, W, Cin, tiles_x, tiles_y, act, gscale};
    hipStream_t s = (hipStream_t)stream;
    if (dx) {
        const int nb = N * D * tiles_y * tiles_x;
        G3_DISPATCH(g3_tail_dx_kernel, nb, a);
    }
    if (dw) {
        const int64_t nvox = (int64_t)N * D * H * W;
        const int parts = g3_parts(nvox);
        const int vpp = (int)cdiv64(nvox, parts);
        const int items = 27 * (Cin >> 3), T = Cout * Cin * 27;
        int ipb = 32;
        while (ipb < items) ipb <<= 1;
        G3_DISPATCH(g3_tail_dw_kernel, parts, a, (int)nvox, vpp, ipb);
        g3_tail_reduce_kernel<<<cdiv(T + Cout, 32), 256, 0, s>>>(ws, parts, T, Cout, dw, db);
    }
    GS_CHECK_LAUNCH("gs_conv3d_tail_bwd");
    return GS_OK;
}
