// The two 7x7 ends of the ResNet generator (reference models_pix2pix/networks.py:340-343 and :371-373): convolutions between
// an fp32 NCHW image of 1..4 channels and a 16-bit NHWC tensor of ANY channel count that is a multiple of 8.  The direct
// kernels of direct.hip keep the whole weight tensor in 32 KB of LDS (3 -> 64 channels at 7x7 is 37 KB) and split a block's
// lanes by a power-of-two channel-chunk count; here the weights are TILED: a block holds the taps of 32 (to_img: 64) of the
// wide side's channels (at most 4 * 49 * 32 floats, 25 KB; 50 KB) and either owns one such tile (grid.y) or walks the tiles
// with its sums in registers.  Three kernels serve the six products, each in two roles (`pad` = 0: the convolution as the reference states it
// on the reflection-padded tensor; `pad` = k - 1 with flipped taps: the full correlation that is its data gradient):
//   gs_conv_ends_to_c16 : image -> 16-bit.   stem forward (+ BatchNorm partial sums)  /  head data gradient
//   gs_conv_ends_to_img : 16-bit -> image.   head forward (+ bias)                    /  stem data gradient
//   gs_conv_ends_wgrad  : sum over pixels of (16-bit pixel row) x (image taps): stem weight gradient / head weight + bias
//                         gradient.  Every thread owns its (channel chunk, tap) sums for a block's pixels -- no reduction
//                         inside the block -- the blocks' slabs are summed in block order in double.  No atomics.
// Weights are the module's own fp32 tensors: w_img_major = 0: [C16][Cimg][k][k] (the stem), 1: [Cimg][C16][k][k] (the head).
#include "common.hpp"

namespace {

constexpr int E_MAXK = 7;
constexpr int E_MAXT = 4 * E_MAXK * E_MAXK;     // taps x image channels
constexpr int E_CW = 32;                        // wide-side channels per weight tile
constexpr int E_TILE = 1024;                    // output pixels per block of to_c16 (one BatchNorm partial row each)
constexpr int E_ICW = 64;                       // to_img: wide-side channels per weight tile = 8 lanes x 16 bytes, one 128-byte row
constexpr int E_IPX = 4;                        // to_img: output pixels per lane (they share every weight read)
constexpr int E_IMG_TILE = 32 * E_IPX;          // to_img: output pixels per block
constexpr int E_WG_CW = 64;                     // wide-side channels per block of the weight gradient
constexpr int E_WG_TPT = 7;                     // taps per thread there: 256 / (64 / 8) = 32 tap lanes, 7 * 32 >= 196
constexpr int E_WG_BLOCKS = 1024;
constexpr int E_DB_BLOCKS = 64;

inline bool e_al(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

struct EArgs {
    const float* img; const unsigned short* t16; const float* w; const float* bias;
    float* out_img; unsigned short* out16; float* bnp; float* slab;
    int N, Cimg, IH, IW, C16, OH, OW, k, pad, flip, w_img_major;
    float gscale; int pix_per_block;
};

__device__ __forceinline__ int64_t e_widx(const EArgs& a, int c16, int cimg, int t) {
    const int kk = a.k * a.k, tf = a.flip ? kk - 1 - t : t;
    return a.w_img_major ? ((int64_t)cimg * a.C16 + c16) * kk + tf : ((int64_t)c16 * a.Cimg + cimg) * kk + tf;
}

// wl[tap = cimg * kk + t][CW] for the channels c0 .. c0 + CW - 1 of the wide side (zeros past C16)
template <int CW>
__device__ __forceinline__ void e_load_tile(const EArgs& a, int c0, float* wl) {
    const int kk = a.k * a.k, T = a.Cimg * kk;
    for (int i = threadIdx.x; i < T * CW; i += 256) {
        const int cl = i % CW, tap = i / CW, c = c0 + cl;
        wl[i] = c < a.C16 ? a.w[e_widx(a, c, tap / kk, tap % kk)] : 0.f;
    }
}

// ---- image -> 16-bit: a thread owns an output pixel and the 32 channels of the block's tile --------------------------------
template <int DT>
__global__ __launch_bounds__(256) void ends_to_c16_kernel(const EArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[E_MAXT * E_CW];
    __shared__ float red[4][2 * E_CW];
    const int c0 = blockIdx.y * E_CW;
    const int ng = (a.C16 - c0 < E_CW ? a.C16 - c0 : E_CW) >> 3;       // 8-channel groups of this tile (uniform)
    e_load_tile<E_CW>(a, c0, wl);
    __syncthreads();
    const int64_t M = (int64_t)a.N * a.OH * a.OW;
    const int64_t m0 = (int64_t)blockIdx.x * E_TILE;
    const int64_t plane = (int64_t)a.IH * a.IW;
    float s1[4][8], s2[4][8];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 8; ++i) { s1[g][i] = 0.f; s2[g][i] = 0.f; }
    for (int j = 0; j < E_TILE / 256; ++j) {
        const int64_t m = m0 + j * 256 + threadIdx.x;
        if (m >= M) break;
        const int ox = (int)(m % a.OW);
        const int64_t r = m / a.OW;
        const int oy = (int)(r % a.OH);
        const int n = (int)(r / a.OH);
        float acc[4][8];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
        int tap = 0;
        for (int ci = 0; ci < a.Cimg; ++ci) {
            const float* xc = a.img + ((int64_t)n * a.Cimg + ci) * plane;
            for (int ty = 0; ty < a.k; ++ty) {
                const int iy = oy + ty - a.pad;
                for (int tx = 0; tx < a.k; ++tx, ++tap) {
                    const int ix = ox + tx - a.pad;
                    float xv = 0.f;
                    if ((unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW) xv = xc[(int64_t)iy * a.IW + ix];
                    const float* wp = wl + tap * E_CW;
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (g < ng) {
#pragma unroll
                            for (int i = 0; i < 8; ++i) acc[g][i] += xv * wp[g * 8 + i];
                        }
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (g < ng) {
#pragma unroll
                for (int i = 0; i < 8; ++i) { s1[g][i] += acc[g][i]; s2[g][i] += acc[g][i] * acc[g][i]; }
                *reinterpret_cast<uint4*>(a.out16 + m * a.C16 + c0 + g * 8) = pack8<DT>(acc[g]);
            }
    }
    if (a.bnp) {                                                       // [tile][2][C16]: sum, sum of squares (fixed order)
        const int wv = threadIdx.x >> 6;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float t1 = wave_sum(s1[g][i]), t2 = wave_sum(s2[g][i]);
                if ((threadIdx.x & 63) == 0) { red[wv][g * 8 + i] = t1; red[wv][E_CW + g * 8 + i] = t2; }
            }
        __syncthreads();
        if (threadIdx.x < 2 * E_CW) {
            const int cl = threadIdx.x % E_CW, which = threadIdx.x / E_CW;
            if (c0 + cl < a.C16)
                a.bnp[((int64_t)blockIdx.x * 2 + which) * a.C16 + c0 + cl] =
                    (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        }
    }
}

// ---- 16-bit -> image: eight lanes share an output pixel, one 16-byte chunk of its 128-byte row each (a wave reads eight whole rows
// per load); a lane keeps the sums of E_IPX pixels, 32 apart, which share every weight read from LDS; the block walks the weight
// tiles of 64 channels, and the eight lanes' sums meet in three shuffles at the end --------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void ends_to_img_kernel(const EArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[E_MAXT * E_ICW];
    const int kk = a.k * a.k;
    const int g = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const int64_t M = (int64_t)a.N * a.OH * a.OW;
    int oy[E_IPX], ox[E_IPX], nn[E_IPX];
    bool valid[E_IPX];
#pragma unroll
    for (int q = 0; q < E_IPX; ++q) {
        const int64_t m = (int64_t)blockIdx.x * E_IMG_TILE + q * 32 + slot;
        valid[q] = m < M;
        const int64_t mm = valid[q] ? m : 0;
        ox[q] = (int)(mm % a.OW);
        const int64_t r = mm / a.OW;
        oy[q] = (int)(r % a.OH);
        nn[q] = (int)(r / a.OH);
    }
    float acc[E_IPX][4];
#pragma unroll
    for (int q = 0; q < E_IPX; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[q][c] = 0.f;
    for (int c0 = 0; c0 < a.C16; c0 += E_ICW) {
        const int ng = (a.C16 - c0 < E_ICW ? a.C16 - c0 : E_ICW) >> 3;
        __syncthreads();
        e_load_tile<E_ICW>(a, c0, wl);
        __syncthreads();
        if (g >= ng) continue;                                        // (uniform trip count: every lane meets every barrier)
        for (int ty = 0; ty < a.k; ++ty)
            for (int tx = 0; tx < a.k; ++tx) {
                const int t = ty * a.k + tx;
                float wr[4][8];
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < a.Cimg) {
                        const float* wp = wl + (c * kk + t) * E_ICW + g * 8;
#pragma unroll
                        for (int i = 0; i < 8; ++i) wr[c][i] = wp[i];
                    }
#pragma unroll
                for (int q = 0; q < E_IPX; ++q) {
                    const int iy = oy[q] + ty - a.pad, ix = ox[q] + tx - a.pad;
                    if (!valid[q] || (unsigned)iy >= (unsigned)a.IH || (unsigned)ix >= (unsigned)a.IW) continue;
                    float v[8];
                    unpack8<DT>(*reinterpret_cast<const uint4*>(a.t16 + (((int64_t)nn[q] * a.IH + iy) * a.IW + ix) * a.C16 + c0 + g * 8), v);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < a.Cimg) {
                            float s = 0.f;
#pragma unroll
                            for (int i = 0; i < 8; ++i) s += v[i] * wr[c][i];
                            acc[q][c] += s;
                        }
                }
            }
    }
#pragma unroll
    for (int q = 0; q < E_IPX; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < a.Cimg) {                                         // (uniform)
                float s = acc[q][c];
                s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
                if (g == 0 && valid[q])
                    a.out_img[(((int64_t)nn[q] * a.Cimg + c) * a.OH + oy[q]) * a.OW + ox[q]] = s * a.gscale + (a.bias ? a.bias[c] : 0.f);
            }
}

// ---- weight gradient: IH x IW is the 16-bit tensor's plane, OH x OW the image's ---------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void ends_wgrad_kernel(const EArgs a) {
    const int kk = a.k * a.k, T = a.Cimg * kk;
    const int c0 = blockIdx.y * E_WG_CW;
    const int nch = (a.C16 - c0 < E_WG_CW ? a.C16 - c0 : E_WG_CW) >> 3;       // 1..8
    const int L = 256 / nch;                                                   // tap lanes
    const int ch = threadIdx.x % nch, tl = threadIdx.x / nch;
    const int M = a.N * a.IH * a.IW;                                           // host guarantees < 2^31
    const int m0 = blockIdx.x * a.pix_per_block;
    const int m1 = m0 + a.pix_per_block < M ? m0 + a.pix_per_block : M;
    const int plane = a.OH * a.OW;
    float acc[E_WG_TPT][8];
    int toff[E_WG_TPT], tdy[E_WG_TPT], tdx[E_WG_TPT];
    bool tok[E_WG_TPT];
#pragma unroll
    for (int j = 0; j < E_WG_TPT; ++j) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j][i] = 0.f;
        const int tap = tl + j * L;
        tok[j] = tl < L && tap < T;
        const int tp = tok[j] ? tap : 0;
        const int ci = tp / kk, t = tp - ci * kk, ty = t / a.k;
        toff[j] = ci * plane; tdy[j] = ty - a.pad; tdx[j] = t - ty * a.k - a.pad;
    }
    if (tl < L && tl < T) {
        int ax = m0 % a.IW, r = m0 / a.IW;
        int ay = r % a.IH, n = r / a.IH;
        for (int m = m0; m < m1; ++m) {
            float g[8];
            unpack8<DT>(*reinterpret_cast<const uint4*>(a.t16 + (int64_t)m * a.C16 + c0 + ch * 8), g);
            const float* bn = a.img + (int64_t)n * a.Cimg * plane;
#pragma unroll
            for (int j = 0; j < E_WG_TPT; ++j) {
                const int by = ay + tdy[j], bx = ax + tdx[j];
                const bool ok = tok[j] && (unsigned)by < (unsigned)a.OH && (unsigned)bx < (unsigned)a.OW;
                const float xv = ok ? bn[toff[j] + by * a.OW + bx] : 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[j][i] += g[i] * xv;
            }
            if (++ax == a.IW) { ax = 0; if (++ay == a.IH) { ay = 0; ++n; } }
        }
    }
    float* slab = a.slab + (int64_t)blockIdx.x * a.C16 * T;
#pragma unroll
    for (int j = 0; j < E_WG_TPT; ++j)
        if (tok[j]) {
            const int tap = tl + j * L, ci = tap / kk, t = tap - ci * kk;
#pragma unroll
            for (int i = 0; i < 8; ++i) slab[e_widx(a, c0 + ch * 8 + i, ci, t)] = acc[j][i];
        }
}

// out[j] = gscale * sum_b slab[b * stride + j], b ascending in four interleaved double sums
__global__ __launch_bounds__(256) void ends_slab_reduce_kernel(const float* __restrict__ slab, int nb, int64_t stride, int n,
                                                               float gscale, float* out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int b = 0;
    for (; b + 3 < nb; b += 4)
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += (double)slab[(int64_t)(b + u) * stride + j];
    for (; b < nb; ++b) s[0] += (double)slab[(int64_t)b * stride + j];
    out[j] = (float)(((s[0] + s[1]) + (s[2] + s[3])) * (double)gscale);
}

// bias gradient partials [block][4]: block b of channel c sums its strided share of img[:, c]
__global__ __launch_bounds__(256) void ends_bias_partial_kernel(const float* __restrict__ img, int N, int C, int64_t plane,
                                                                float* part) {
    __shared__ float red[4];
    const int c = blockIdx.y;
    float s = 0.f;
    for (int n = 0; n < N; ++n) {
        const float* p = img + ((int64_t)n * C + c) * plane;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < plane; i += (int64_t)gridDim.x * 256) s += p[i];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x * 4 + c] = (red[0] + red[1]) + (red[2] + red[3]);
}

int e_wgrad_ppb(int64_t M) {
    int64_t ppb = cdiv64(M, E_WG_BLOCKS);
    return (int)(ppb < 64 ? 64 : ppb);
}

// img [N,Cimg,IH,IW] and t16 [N,TH,TW,C16] of a k x k convolution with `pad` zeros on the image (to_c16) / on t16 (to_img)
int e_check(const char* who, int N, int Cimg, int C16, int k, int pad, int flip, int w_img_major, int dtype) {
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "%s: bad dtype", who);
    GS_CHECK_ARG(N > 0 && Cimg >= 1 && Cimg <= 4, "%s: the image side has 1..4 channels, got %d", who, Cimg);
    GS_CHECK_ARG(C16 >= 8 && C16 % 8 == 0, "%s: the 16-bit side's channels must be a multiple of 8, got %d", who, C16);
    GS_CHECK_ARG(k >= 1 && k <= E_MAXK && pad >= 0 && pad < k, "%s: k=%d pad=%d out of range (k <= %d, pad < k)", who, k, pad, E_MAXK);
    GS_CHECK_ARG((flip == 0 || flip == 1) && (w_img_major == 0 || w_img_major == 1), "%s: flip / w_img_major are 0 or 1", who);
    return GS_OK;
}

}  // namespace

extern "C" int gs_conv_ends_mtiles(int N, int OH, int OW) { return (int)cdiv64((int64_t)N * OH * OW, E_TILE); }

extern "C" int gs_conv_ends_to_c16(const float* img, const float* w, void* out, float* bn_partials, int N, int Cimg, int IH, int IW,
                                   int C16, int OH, int OW, int k, int pad, int flip, int w_img_major, int dtype, void* stream) {
    int rc = e_check("gs_conv_ends_to_c16", N, Cimg, C16, k, pad, flip, w_img_major, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(img && w && out && e_al(img, 4) && e_al(w, 4) && e_al(out, 16) && e_al(bn_partials, 4),
                 "gs_conv_ends_to_c16: null or misaligned pointer");
    GS_CHECK_ARG(IH > 0 && IW > 0 && OH == IH + 2 * pad - k + 1 && OW == IW + 2 * pad - k + 1 && OH > 0 && OW > 0,
                 "gs_conv_ends_to_c16: output size mismatch");
    GS_CHECK_ARG((int64_t)N * OH * OW < 2147483647LL - E_TILE, "gs_conv_ends_to_c16: too many pixels");
    EArgs a{};
    a.img = img; a.w = w; a.out16 = (unsigned short*)out; a.bnp = bn_partials;
    a.N = N; a.Cimg = Cimg; a.IH = IH; a.IW = IW; a.C16 = C16; a.OH = OH; a.OW = OW; a.k = k; a.pad = pad; a.flip = flip;
    a.w_img_major = w_img_major;
    const dim3 grid(gs_conv_ends_mtiles(N, OH, OW), cdiv(C16, E_CW));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GS_F16) ends_to_c16_kernel<GS_F16><<<grid, 256, 0, s>>>(a);
    else ends_to_c16_kernel<GS_BF16><<<grid, 256, 0, s>>>(a);
    GS_CHECK_LAUNCH("gs_conv_ends_to_c16");
    return GS_OK;
}

extern "C" int gs_conv_ends_to_img(const void* t16, const float* w, const float* bias, float* out, int N, int IH, int IW, int C16,
                                   int Cimg, int OH, int OW, int k, int pad, int flip, int w_img_major, float gscale, int dtype,
                                   void* stream) {
    int rc = e_check("gs_conv_ends_to_img", N, Cimg, C16, k, pad, flip, w_img_major, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(t16 && w && out && e_al(t16, 16) && e_al(w, 4) && e_al(out, 4) && e_al(bias, 4),
                 "gs_conv_ends_to_img: null or misaligned pointer");
    GS_CHECK_ARG(IH > 0 && IW > 0 && OH == IH + 2 * pad - k + 1 && OW == IW + 2 * pad - k + 1 && OH > 0 && OW > 0,
                 "gs_conv_ends_to_img: output size mismatch");
    GS_CHECK_ARG((int64_t)N * OH * OW < 2147483647LL - E_IMG_TILE, "gs_conv_ends_to_img: too many pixels");
    EArgs a{};
    a.t16 = (const unsigned short*)t16; a.w = w; a.bias = bias; a.out_img = out; a.gscale = gscale;
    a.N = N; a.Cimg = Cimg; a.IH = IH; a.IW = IW; a.C16 = C16; a.OH = OH; a.OW = OW; a.k = k; a.pad = pad; a.flip = flip;
    a.w_img_major = w_img_major;
    const int nb = (int)cdiv64((int64_t)N * OH * OW, E_IMG_TILE);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GS_F16) ends_to_img_kernel<GS_F16><<<nb, 256, 0, s>>>(a);
    else ends_to_img_kernel<GS_BF16><<<nb, 256, 0, s>>>(a);
    GS_CHECK_LAUNCH("gs_conv_ends_to_img");
    return GS_OK;
}

extern "C" int64_t gs_conv_ends_wgrad_ws_floats(int N, int TH, int TW, int Cimg, int C16, int k) {
    const int64_t M = (int64_t)N * TH * TW;
    return cdiv64(M, e_wgrad_ppb(M)) * C16 * Cimg * k * k + E_DB_BLOCKS * 4;
}

extern "C" int gs_conv_ends_wgrad(const void* t16, const float* img, float* dw, float* db, float* ws, int N, int TH, int TW,
                                  int C16, int Cimg, int BH, int BW, int k, int pad, int flip, int w_img_major, float gscale,
                                  int dtype, void* stream) {
    int rc = e_check("gs_conv_ends_wgrad", N, Cimg, C16, k, pad, flip, w_img_major, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(t16 && img && dw && ws && e_al(t16, 16) && e_al(img, 4) && e_al(dw, 4) && e_al(db, 4) && e_al(ws, 4),
                 "gs_conv_ends_wgrad: null or misaligned pointer");
    GS_CHECK_ARG(TH > 0 && TW > 0 && BH == TH + k - 1 - 2 * pad && BW == TW + k - 1 - 2 * pad && BH > 0 && BW > 0,
                 "gs_conv_ends_wgrad: plane size mismatch");
    const int64_t M = (int64_t)N * TH * TW;
    GS_CHECK_ARG(M < 2147483647LL - (1 << 22) && (int64_t)Cimg * BH * BW < 2147483647LL, "gs_conv_ends_wgrad: too many pixels");
    EArgs a{};
    a.t16 = (const unsigned short*)t16; a.img = img; a.slab = ws;
    a.N = N; a.Cimg = Cimg; a.IH = TH; a.IW = TW; a.C16 = C16; a.OH = BH; a.OW = BW; a.k = k; a.pad = pad; a.flip = flip;
    a.w_img_major = w_img_major;
    a.pix_per_block = e_wgrad_ppb(M);
    const int nb = (int)cdiv64(M, a.pix_per_block);
    const int n = C16 * Cimg * k * k;
    const dim3 grid(nb, cdiv(C16, E_WG_CW));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GS_F16) ends_wgrad_kernel<GS_F16><<<grid, 256, 0, s>>>(a);
    else ends_wgrad_kernel<GS_BF16><<<grid, 256, 0, s>>>(a);
    ends_slab_reduce_kernel<<<cdiv(n, 256), 256, 0, s>>>(ws, nb, n, n, gscale, dw);
    if (db) {
        float* part = ws + (int64_t)nb * n;
        ends_bias_partial_kernel<<<dim3(E_DB_BLOCKS, Cimg), 256, 0, s>>>(img, N, Cimg, (int64_t)BH * BW, part);
        ends_slab_reduce_kernel<<<1, 256, 0, s>>>(part, E_DB_BLOCKS, 4, Cimg, gscale, db);
    }
    GS_CHECK_LAUNCH("gs_conv_ends_wgrad");
    return GS_OK;
}
