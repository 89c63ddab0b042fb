// The one-channel head of the 3-D Pix2Pix discriminators (GenSeg-3D/models/networks.py:806-890 with a 3-D norm layer): the last conv of
// NLayerDiscriminator, Conv3d(C, 1, k4, s1, p1), :850, and of PixelDiscriminator, Conv3d(C, 1, k1), :884.  (Their image-side conv is
// the R = 3 case of csrc/ends_img.hip.)  Volumes are stacks of depth slices, as everywhere else: 16-bit [N*D,H,W,Cin], Cin a
// multiple of 8 up to 1024, fp32 weights [1][Cin][k][k][k] -> fp32 logits [N,1,OD,OH,OW]; the contract of gs_conv_smallcout_fwd /
// _bwd.  The output volume is tiny (6^3 at a 64^3 crop) under a K of up to 65536, so the k4 forward is a REDUCTION: one block per
// logit, the 256 threads take (tap, 8-channel group) items, taps fastest (adjacent lanes read adjacent weights), and the block sum
// has a fixed order.  k1: 8 lanes per voxel.  Backward: dz 16-bit = sum over taps dl * w, rounded once (k4: grid.y = the 8-channel
// group, so its 512 weights are wave-uniform; k1: a thread per (voxel, group)); dw and db += gscale * sums, through per-part slabs
// (a thread owns one (tap, group) item = 8 weights and walks the part's logits) added in part order by a second launch.
#include "common.hpp"

namespace {

struct E3HArgs {
    const unsigned short* x; const float* w; const float* bias; const float* dl; float* y; unsigned short* dz; float* ws;
    int N, D, H, W, Cin, OD, OH, OW;
};

// k4 / s1 / p1: one block per logit; item = (8-channel group, tap), taps fastest
template <int DT>
__global__ __launch_bounds__(256) void e3_head_fwd_k4_kernel(const E3HArgs a) {
    __shared__ float red[4];
    int v = blockIdx.x;
    const int ox = v % a.OW; v /= a.OW;
    const int oy = v % a.OH; v /= a.OH;
    const int od = v % a.OD;
    const int n = v / a.OD;
    const int items = (a.Cin >> 3) * 64;
    float s = 0.f;
    for (int it = threadIdx.x; it < items; it += 256) {
        const int tap = it & 63, g = it >> 6;
        const int z = od - 1 + (tap >> 4), y = oy - 1 + ((tap >> 2) & 3), xx = ox - 1 + (tap & 3);
        if ((unsigned)z >= (unsigned)a.D || (unsigned)y >= (unsigned)a.H || (unsigned)xx >= (unsigned)a.W) continue;
        float f[8];
        unpack8<DT>(*reinterpret_cast<const uint4*>(a.x + ((((int64_t)n * a.D + z) * a.H + y) * a.W + xx) * a.Cin + g * 8), f);
        const float* wp = a.w + (int64_t)g * 512 + tap;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += f[i] * wp[i * 64];
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) a.y[blockIdx.x] = s + (a.bias ? a.bias[0] : 0.f);
}

// k1: 8 lanes per voxel, each over every eighth 8-channel group; the three exchanges add in a fixed order
template <int DT>
__global__ __launch_bounds__(256) void e3_head_fwd_k1_kernel(const E3HArgs a, int nvox) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int v = gid >> 3, sub = gid & 7;
    const int G = a.Cin >> 3;
    float s = 0.f;
    if (v < nvox)
        for (int g = sub; g < G; g += 8) {
            float f[8];
            unpack8<DT>(*reinterpret_cast<const uint4*>(a.x + (int64_t)v * a.Cin + g * 8), f);
            const float* wp = a.w + g * 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) s += f[i] * wp[i];
        }
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 1, 64);
    if (sub == 0 && v < nvox) a.y[v] = s + (a.bias ? a.bias[0] : 0.f);
}

// dz, k4: grid.y = the 8-channel group (its 8 x 64 weights are wave-uniform), a thread owns one input voxel
template <int DT>
__global__ __launch_bounds__(256) void e3_head_dz_k4_kernel(const E3HArgs a) {
    const int g = blockIdx.y;
    const float* wg = a.w + (int64_t)g * 512;
    const int total = a.N * a.D * a.H * a.W;               // host guarantees < 2^31 - the grid's stride
    for (int v = blockIdx.x * 256 + threadIdx.x; v < total; v += gridDim.x * 256) {
        const int xx = v % a.W;
        int r = v / a.W;
        const int y = r % a.H; r /= a.H;
        const int z = r % a.D;
        const int n = r / a.D;
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        // the forward reads input slice z at tap kz of output slice z + 1 - kz
        for (int kz = 0; kz < 4; ++kz) {
            const int od = z + 1 - kz;
            if ((unsigned)od >= (unsigned)a.OD) continue;
            for (int ky = 0; ky < 4; ++ky) {
                const int oy = y + 1 - ky;
                if ((unsigned)oy >= (unsigned)a.OH) continue;
                const float* dlp = a.dl + (((int64_t)n * a.OD + od) * a.OH + oy) * a.OW;
#pragma unroll
                for (int kx = 0; kx < 4; ++kx) {
                    const int ox = xx + 1 - kx;
                    if ((unsigned)ox >= (unsigned)a.OW) continue;
                    const float d = dlp[ox];
                    const float* wp = wg + (kz * 4 + ky) * 4 + kx;
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[i] += d * wp[i * 64];
                }
            }
        }
        st16(a.dz + (int64_t)v * a.Cin + g * 8, pack8<DT>(acc));
    }
}

// dz, k1: a thread per (voxel, 8-channel group), groups fastest
template <int DT>
__global__ __launch_bounds__(256) void e3_head_dz_k1_kernel(const E3HArgs a, int64_t nitem) {
    const int G = a.Cin >> 3;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < nitem; it += (int64_t)gridDim.x * 256) {
        const int64_t v = it / G;
        const int g = (int)(it - v * G);
        const float d = a.dl[v];
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = d * a.w[g * 8 + i];
        st16(a.dz + v * a.Cin + g * 8, pack8<DT>(o));
    }
}

// per-part slabs of dw (and, in their last element, of db): block (part, item tile); a thread owns item = (tap, 8-channel group),
// groups fastest, and walks the part's logits v0 + sub, + SUB, ...; the SUB partial sums are added in order
template <int DT, int K>
__global__ __launch_bounds__(256) void e3_head_dw_kernel(const E3HArgs a, int nvox, int vpp, int ipb) {
    constexpr int KKK = K * K * K, P = K == 4 ? 1 : 0;
    __shared__ float red[256 * 8];
    const int G = a.Cin >> 3, items = KKK * G, T = a.Cin * KKK;
    const int sub_n = 256 / ipb;
    const int v0 = blockIdx.x * vpp, v1 = v0 + vpp < nvox ? v0 + vpp : nvox;
    const int il = threadIdx.x % ipb, sub = threadIdx.x / ipb;
    const int item = blockIdx.y * ipb + il;
    const bool live = item < items;
    const int g = item % G, tap = item / G;
    const int kz = tap / (K * K), ky = (tap / K) % K, kx = tap % K;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    if (live)
        for (int v = v0 + sub; v < v1; v += sub_n) {
            const int ox = v % a.OW;
            int r = v / a.OW;
            const int oy = r % a.OH; r /= a.OH;
            const int od = r % a.OD;
            const int n = r / a.OD;
            const int z = od - P + kz, y = oy - P + ky, xx = ox - P + kx;
            if ((unsigned)z >= (unsigned)a.D || (unsigned)y >= (unsigned)a.H || (unsigned)xx >= (unsigned)a.W) continue;
            const float d = a.dl[v];
            float f[8];
            unpack8<DT>(*reinterpret_cast<const uint4*>(a.x + ((((int64_t)n * a.D + z) * a.H + y) * a.W + xx) * a.Cin + g * 8), f);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += d * f[i];
        }
    if (sub_n > 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[threadIdx.x * 8 + i] = acc[i];
        __syncthreads();
        if (sub == 0)
            for (int s = 1; s < sub_n; ++s)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] += red[(s * ipb + il) * 8 + i];
    }
    float* const slab = a.ws + (int64_t)blockIdx.x * (T + 1);
    if (sub == 0 && live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) slab[(g * 8 + i) * KKK + tap] = acc[i];
    }
    if (blockIdx.y == 0 && threadIdx.x < 64) {             // the part's share of db: one wave, fixed order
        float s = 0.f;
        for (int v = v0 + (int)threadIdx.x; v < v1; v += 64) s += a.dl[v];
        s = wave_sum(s);
        if (threadIdx.x == 0) slab[T] = s;
    }
}

// dw[i] += gscale * sum over the parts in order; element T is db
__global__ __launch_bounds__(256) void e3_head_reduce_kernel(const float* ws, int nparts, int T, float gscale, float* dw, float* db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > T) return;
    float s = 0.f;
    for (int p = 0; p < nparts; ++p) s += ws[(int64_t)p * (T + 1) + i];
    if (i < T) dw[i] += gscale * s;
    else db[0] += gscale * s;
}

int e3_head_parts(int64_t nvox) {
    const int64_t p = cdiv64(nvox, 64);
    return (int)(p < 1 ? 1 : p > 256 ? 256 : p);
}

int e3_head_check(const char* who, const void* x16, const float* w, int N, int D, int H, int W, int Cin, int OD, int OH, int OW, int k,
                  int pad, int dtype) {
    GS_CHECK_ARG(x16 && w, "%s: null pointer", who);
    GS_CHECK_ARG(((uintptr_t)x16 & 15) == 0 && ((uintptr_t)w & 3) == 0,
                 "%s: the 16-bit tensor must be 16-byte aligned, the fp32 tensors 4-byte aligned", who);
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "%s: bad dtype", who);
    GS_CHECK_ARG(N > 0 && D > 0 && H > 0 && W > 0 && OD > 0 && OH > 0 && OW > 0, "%s: bad dims", who);
    if (Cin < 8 || Cin > 1024 || Cin % 8 != 0 || !((k == 4 && pad == 1) || (k == 1 && pad == 0))) return GS_EUNSUPPORTED;
    const int e = 2 * pad - k + 1;
    GS_CHECK_ARG(OD == D + e && OH == H + e && OW == W + e, "%s: output size mismatch", who);
    GS_CHECK_ARG((int64_t)N * D * H * W < 2147483647LL / 8 - 4096 * 256, "%s: too many voxels", who);
    return GS_OK;
}

}  // namespace

extern "C" int gs_conv3d_head_fwd(const void* x, const float* w, const float* bias, float* y, int N, int D, int H, int W, int Cin, int OD,
                                  int OH, int OW, int k, int pad, int dtype, void* stream) {
    int rc = e3_head_check("gs_conv3d_head_fwd", x, w, N, D, H, W, Cin, OD, OH, OW, k, pad, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(y && (((uintptr_t)y | (uintptr_t)bias) & 3) == 0, "gs_conv3d_head_fwd: null or misaligned logits / bias");
    E3HArgs a{(const unsigned short*)x, w, bias, nullptr, y, nullptr, nullptr, N, D, H, W, Cin, OD, OH, OW};
    hipStream_t s = (hipStream_t)stream;
    const int nvox = N * OD * OH * OW;
    if (k == 4) {
        if (dtype == GS_F16) e3_head_fwd_k4_kernel<GS_F16><<<nvox, 256, 0, s>>>(a);
        else e3_head_fwd_k4_kernel<GS_BF16><<<nvox, 256, 0, s>>>(a);
    } else {
        const int nb = (int)cdiv64((int64_t)nvox * 8, 256);
        if (dtype == GS_F16) e3_head_fwd_k1_kernel<GS_F16><<<nb, 256, 0, s>>>(a, nvox);
        else e3_head_fwd_k1_kernel<GS_BF16><<<nb, 256, 0, s>>>(a, nvox);
    }
    GS_CHECK_LAUNCH("gs_conv3d_head_fwd");
    return GS_OK;
}

extern "C" int64_t gs_conv3d_head_bwd_ws_floats(int N, int OD, int OH, int OW, int Cin, int k) {
    if (N <= 0 || OD <= 0 || OH <= 0 || OW <= 0 || Cin <= 0 || (k != 4 && k != 1)) return 0;
    return (int64_t)e3_head_parts((int64_t)N * OD * OH * OW) * ((int64_t)Cin * k * k * k + 1);
}

extern "C" int gs_conv3d_head_bwd(const void* x, const float* w, const float* dl, void* dz, float* dw, float* db, float* ws, int N, int D,
                                  int H, int W, int Cin, int OD, int OH, int OW, int k, int pad, float gscale, int dtype, void* stream) {
    const void* any16 = x ? x : dz;
    int rc = e3_head_check("gs_conv3d_head_bwd", any16, w, N, D, H, W, Cin, OD, OH, OW, k, pad, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(dl && ((uintptr_t)dl & 3) == 0, "gs_conv3d_head_bwd: null or misaligned dl");
    GS_CHECK_ARG((((uintptr_t)x | (uintptr_t)dz) & 15) == 0, "gs_conv3d_head_bwd: x and dz must be 16-byte aligned");
    GS_CHECK_ARG((dw == nullptr) == (db == nullptr) && (((uintptr_t)dw | (uintptr_t)db) & 3) == 0,
                 "gs_conv3d_head_bwd: dw and db go together, 4-byte aligned");
    GS_CHECK_ARG(dw == nullptr || (x && ws && ((uintptr_t)ws & 3) == 0), "gs_conv3d_head_bwd: the weight gradient needs x and a workspace");
    GS_CHECK_ARG(dz || dw, "gs_conv3d_head_bwd: nothing to compute");
    E3HArgs a{(const unsigned short*)x, w, nullptr, dl, nullptr, (unsigned short*)dz, ws, N, D, H, W, Cin, OD, OH, OW};
    hipStream_t s = (hipStream_t)stream;
    const int G = Cin >> 3;
    if (dz) {
        const int64_t nin = (int64_t)N * D * H * W;
        if (k == 4) {
            const int64_t nb = cdiv64(nin, 256);
            const dim3 grid((int)(nb < 4096 ? nb : 4096), G);
            if (dtype == GS_F16) e3_head_dz_k4_kernel<GS_F16><<<grid, 256, 0, s>>>(a);
            else e3_head_dz_k4_kernel<GS_BF16><<<grid, 256, 0, s>>>(a);
        } else {
            const int64_t nb = cdiv64(nin * G, 256);
            const int grid = (int)(nb < 4096 ? nb : 4096);
            if (dtype == GS_F16) e3_head_dz_k1_kernel<GS_F16><<<grid, 256, 0, s>>>(a, nin * G);
            else e3_head_dz_k1_kernel<GS_BF16><<<grid, 256, 0, s>>>(a, nin * G);
        }
    }
    if (dw) {
        const int nvox = N * OD * OH * OW;
        const int parts = e3_head_parts(nvox), vpp = cdiv(nvox, parts);
        const int items = G * k * k * k, T = Cin * k * k * k;
        int ipb = 1;
        while (ipb < items && ipb < 256) ipb <<= 1;
        const dim3 grid(parts, cdiv(items, ipb));
#define E3_HDW(DT)                                                                           \
    do {                                                                                     \
        if (k == 4) e3_head_dw_kernel<DT, 4><<<grid, 256, 0, s>>>(a, nvox, vpp, ipb);        \
        else e3_head_dw_kernel<DT, 1><<<grid, 256, 0, s>>>(a, nvox, vpp, ipb);               \
    } while (0)
        if (dtype == GS_F16) E3_HDW(GS_F16);
        else E3_HDW(GS_BF16);
#undef E3_HDW
        e3_head_reduce_kernel<<<cdiv(T + 1, 256), 256, 0, s>>>(ws, parts, T, gscale, dw, db);
    }
    GS_CHECK_LAUNCH("gs_conv3d_head_bwd");
    return GS_OK;
}
