// The image-side conv of the Pix2Pix networks for 5..16 image channels (models_pix2pix/networks.py:640 PatchGAN model.0, :686
// PixelDiscriminator net.0, :582 the U-Net generator's outermost down-conv): fp32 NCHW image [N,Cin,IH,IW] and fp32 weights in the
// reference layout [Cout][Cin][k][k] <-> a dense 16-bit NHWC tensor [N,OH,OW,Cout], Cout any multiple of 8 up to 128, in the two
// geometries these layers have: k4 / stride 2 / pad 1 and k1 / stride 1 / pad 0.  (csrc/direct.hip covers Cin 1..4 and keeps the
// whole weight tensor in LDS; at 16 channels x 16 taps x 128 outputs that is 32768 floats, so here it is tiled.)
//
// As in csrc/stem_wide.hip the image is NOT rounded to 16 bits and the products are fp32 x fp32 accumulated in fp32 on
// v_mfma_f32_32x32x2_f32 (bit-identical to a k-ordered fmaf chain).
//
//   gs_conv_imgwide_fwd    one block per 8 x 32 OUTPUT pixels.  Per chunk of CC input channels (4 for k4: K = 64; 16 for k1) it stages
//                          the patch's fp32 halo (18 x 66 for k4 -- the zeros of the pad come from the bounds test here, once per halo
//                          element) and the weight slab [k][Cout tile rows] (row stride 32 NT + 1).  A stride-2 halo row is stored
//                          de-interleaved (even columns, then odd columns): the 32 lanes of an MFMA B operand, which are 32 adjacent
//                          OUTPUT columns, then read 32 adjacent floats.  A operand = weights (rows = 32 output channels, permuted so
//                          that register g of lane half h is channel 16 h + g), B operand = pixels: a lane ends with one pixel and
//                          whole 16-byte channel groups.  Wave w owns patch rows 2w, 2w + 1 and every channel tile.  Epilogue: + bias,
//                          LeakyReLU(0.2) or none, round once, 16-byte stores.
//   gs_conv_imgwide_wgrad  dW = gscale * sum over pixels dy (x) x-taps, also on the fp32 MFMA: A = dy (rows = 32 output channels, k =
//                          two pixels), B = the image at (pixel, tap) (columns = 32 taps = 2 channels x 16 taps for k4).  grid.y walks
//                          chunks of 8 channels (k4: 4 tap tiles, one per wave, each wave over all 128 pixels of a 4 x 32 patch) or is
//                          1 (k1: one tap tile, the four waves take a quarter of the pixels each).  A block walks patches blockIdx.x,
//                          + gridDim.x, ... with its accumulators in registers and writes ONE slab per (block, pixel part); a second
//                          launch adds the slabs in index order.  No atomics: two runs give equal bits.
//   gs_conv_imgwide_dgrad  dx fp32 NCHW = gscale * conv_transpose(dy, w).  For k4/s2 each input pixel has 2 x 2 taps fixed by its
//                          parity class: grid.y = the 4 classes, the block holds that class's 4 taps x Cout x Cin weights in LDS
//                          (at most 8192 floats) and a thread owns one input pixel and all its channels (wave-uniform LDS reads).
#include "common.hpp"

namespace {

constexpr int EW_PW = 32;                         // output columns of a patch (= MFMA columns)
constexpr int EW_FPH = 8, EW_WPH = 4;             // output rows of a forward / weight-gradient patch
constexpr int EW_WGRID = 256;                     // blocks (per channel chunk) of the weight gradient

template <int K>
struct EWGeo {
    static constexpr int S = K == 4 ? 2 : 1, P = K == 4 ? 1 : 0, KK = K * K;
    static constexpr int HC = (EW_PW - 1) * S + K;                           // halo columns: 66 / 32
    // position of halo column hx in its row: stride 2 stores the even columns first, then the odd ones
    static __device__ __forceinline__ int col(int hx) { return S == 2 ? (hx & 1) * (HC / 2) + (hx >> 1) : hx; }
};

// ------------------------------------------------------------------------------------------------ forward
struct EWFArgs {
    const float* x; const float* w; const float* bias; unsigned short* y;
    int N, Cin, IH, IW, Cout, OH, OW, tiles_x, tiles_y, act;
};

template <int DT, int NT, int K>
__global__ __launch_bounds__(256) void ew_fwd_kernel(const EWFArgs a) {
    using G = EWGeo<K>;
    constexpr int S = G::S, KK = G::KK, HC = G::HC;
    constexpr int CC = K == 4 ? 4 : 16;                                      // input channels per chunk
    constexpr int HR = (EW_FPH - 1) * S + K, PLANE = HR * HC;                // 18 x 66 / 8 x 32
    constexpr int KC = CC * KK;                                              // K of a full chunk: 64 / 16
    constexpr int WS = NT * 32 + 1;
    static_assert((CC * PLANE + KC * WS) * 4 + KC * 4 <= 64 * 1024, "forward LDS");
    __shared__ float lds[CC * PLANE + KC * WS];                              // halo | weight slab [k][A row]
    __shared__ int koff[KC];
    float* const halo = lds;
    float* const wl = lds + CC * PLANE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    int t = blockIdx.x;
    const int tx = t % a.tiles_x; t /= a.tiles_x;
    const int ty = t % a.tiles_y;
    const int n = t / a.tiles_y;
    const int ox0 = tx * EW_PW, oy0 = ty * EW_FPH;
    const int ix0 = ox0 * S - G::P, iy0 = oy0 * S - G::P;
    if (threadIdx.x < KC) {
        const int k = threadIdx.x, ci = k / KK, tt = k - ci * KK, ky = tt / K;
        koff[k] = ci * PLANE + ky * HC + G::col(tt - K * ky);
    }
    f32x16 acc[2][NT];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[r][nt][g] = 0.f;

    for (int c0 = 0; c0 < a.Cin; c0 += CC) {
        const int cc = a.Cin - c0 < CC ? a.Cin - c0 : CC;
        const int kc = cc * KK, kcp = (kc + 1) & ~1;
        const int planes = cc + (kc & 1);                  // odd K (k1, odd cc < CC): one zero plane under the zero weight row
        __syncthreads();                                   // the previous chunk has been read
        for (int i = threadIdx.x; i < planes * PLANE; i += 256) {
            const int ci = i / PLANE, r = i - ci * PLANE;
            const int hy = r / HC, hx = r - hy * HC;
            const int iy = iy0 + hy, ix = ix0 + hx;
            float v = 0.f;
            if (ci < cc && (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW)
                v = a.x[(((int64_t)n * a.Cin + c0 + ci) * a.IH + iy) * a.IW + ix];
            halo[ci * PLANE + hy * HC + G::col(hx)] = v;
        }
        for (int i = threadIdx.x; i < NT * 32 * kcp; i += 256) {
            const int co = i / kcp, k = i - co * kcp;
            const float v = (k < kc && co < a.Cout) ? a.w[((int64_t)co * a.Cin + c0) * KK + k] : 0.f;
            const int c = co & 31;
            wl[k * WS + (co & ~31) + ((c >> 2) & 3) * 8 + (c >> 4) * 4 + (c & 3)] = v;
        }
        __syncthreads();
        const float* hb = halo + (S * 2 * wave) * HC + li;
        for (int s = 0; s < kcp; s += 2) {
            const int k = s + lh;
            const float* hp = hb + koff[k];
            const float b0 = hp[0], b1 = hp[S * HC];
            const float* wp = wl + k * WS + li;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float aw = wp[nt * 32];
                acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, b0, acc[0][nt], 0, 0, 0);
                acc[1][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, b1, acc[1][nt], 0, 0, 0);
            }
        }
    }

    // the lane holds pixel (oy0 + 2 wave + r, ox0 + li), channels 32 nt + 16 lh + (0..15): two 16-byte groups per tile
    const int ox = ox0 + li;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + 2 * wave + r;
        if (ox < a.OW && oy < a.OH) {
            const int64_t base = (((int64_t)n * a.OH + oy) * a.OW + ox) * a.Cout;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int g8 = 0; g8 < 2; ++g8) {
                    const int ch = nt * 32 + 16 * lh + g8 * 8;
                    if (ch < a.Cout) {
                        float v8[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            float v = acc[r][nt][g8 * 8 + i];
                            if (a.bias) v += a.bias[ch + i];
                            v8[i] = a.act == GS_ACT_LEAKY02 ? (v > 0.f ? v : 0.2f * v) : v;
                        }
                        st16(a.y + base + ch, pack8<DT>(v8));
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct EWWArgs {
    const float* x; const unsigned short* dy; float* ws;
    int N, Cin, IH, IW, Cout, OH, OW, tiles_x, tiles_y, npatch;
};

template <int K> struct EWWGeo {
    static constexpr int CW = K == 4 ? 8 : 16;            // image channels per grid.y chunk
    static constexpr int TT = K == 4 ? 4 : 1;             // 32-tap tiles per chunk (k1: 16 taps in one tile)
    static constexpr int PP = 4 / TT;                     // pixel parts (waves that share a tap tile)
};

template <int DT, int NT, int K>
__global__ __launch_bounds__(256) void ew_wgrad_kernel(const EWWArgs a) {
    using G = EWGeo<K>;
    using GW = EWWGeo<K>;
    constexpr int S = G::S, KK = G::KK, HC = G::HC;
    constexpr int CW = GW::CW, TT = GW::TT, PP = GW::PP;
    constexpr int HR = (EW_WPH - 1) * S + K, PLANE = HR * HC;                // 10 x 66 / 4 x 32
    constexpr int NPIX = EW_WPH * EW_PW;                                     // 128
    constexpr int RS = NT * 32 + 8;                                          // dy row stride (16-bit elements, 16-byte multiple)
    static_assert(CW * PLANE * 4 + NPIX * RS * 2 <= 64 * 1024, "weight-gradient LDS");
    __shared__ float halo[CW * PLANE];
    __shared__ __attribute__((aligned(16))) unsigned short dyl[NPIX * RS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int tt = wave % TT, pp = wave / TT;
    const int c0 = blockIdx.y * CW;
    const int cc = a.Cin - c0 < CW ? a.Cin - c0 : CW;
    const int tap = tt * 32 + li;                          // the lane's B column: tap (ci, ky, kx) of the chunk
    const bool tap_ok = tap < cc * KK;
    int tapoff = 0;                                        // (a dead column reads plane 0: finite values, never stored)
    if (tap_ok) {
        const int ci = tap / KK, r = tap - ci * KK, ky = r / K;
        tapoff = ci * PLANE + ky * HC + G::col(r - K * ky);
    }
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[nt][g] = 0.f;
    const int ngrp = a.Cout >> 3;

    for (int pt = blockIdx.x; pt < a.npatch; pt += gridDim.x) {
        int t = pt;
        const int tx = t % a.tiles_x; t /= a.tiles_x;
        const int ty = t % a.tiles_y;
        const int n = t / a.tiles_y;
        const int ox0 = tx * EW_PW, oy0 = ty * EW_WPH;
        const int ix0 = ox0 * S - G::P, iy0 = oy0 * S - G::P;
        __syncthreads();                                   // the previous patch has been read
        for (int i = threadIdx.x; i < CW * PLANE; i += 256) {
            const int ci = i / PLANE, r = i - ci * PLANE;
            const int hy = r / HC, hx = r - hy * HC;
            const int iy = iy0 + hy, ix = ix0 + hx;
            float v = 0.f;
            if (ci < cc && (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW)
                v = a.x[(((int64_t)n * a.Cin + c0 + ci) * a.IH + iy) * a.IW + ix];
            halo[ci * PLANE + hy * HC + G::col(hx)] = v;
        }
        for (int i = threadIdx.x; i < NPIX * (NT * 4); i += 256) {           // every 16-byte group of the NT * 32 channel columns
            const int p = i / (NT * 4), g = i - p * (NT * 4);
            const int oy = oy0 + (p >> 5), ox = ox0 + (p & 31);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);                            // pixels outside the plane and channels past Cout: zeros
            if (g < ngrp && oy < a.OH && ox < a.OW)
                v = *reinterpret_cast<const uint4*>(a.dy + (((int64_t)n * a.OH + oy) * a.OW + ox) * a.Cout + g * 8);
            *reinterpret_cast<uint4*>(dyl + p * RS + g * 8) = v;
        }
        __syncthreads();
        const int pbeg = pp * (NPIX / PP), pend = pbeg + NPIX / PP;
        for (int p = pbeg + lh; p < pend; p += 2) {
            const float b = halo[tapoff + (S * (p >> 5)) * HC + (p & 31)];
            const unsigned short* dp = dyl + p * RS + li;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Elem<DT>::to_f(dp[nt * 32]), b, acc[nt], 0, 0, 0);
        }
    }
    // accumulator: column = the lane's tap, register g of lane half lh = channel row 8 (g >> 2) + 4 lh + (g & 3) of the tile
    const int T = a.Cin * KK;
    float* const slab = a.ws + ((int64_t)blockIdx.x * PP + pp) * a.Cout * T + c0 * KK + tap;
    if (tap_ok) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int co = nt * 32 + 8 * (g >> 2) + 4 * lh + (g & 3);
                if (co < a.Cout) slab[(int64_t)co * T] = acc[nt][g];
            }
    }
}

// dw[i] = gscale * sum over the slabs, in a fixed order: 32 elements per block, eight threads per element take every eighth slab
// (four independent partial sums each, so that the loads overlap), then one thread adds the eight parts in order
__global__ __launch_bounds__(256) void ew_slab_sum_kernel(const float* ws, int nslab, int n, float gscale, float* dw) {
    __shared__ float red[8][33];
    const int e = threadIdx.x & 31, part = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + e;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (i < n) {
        int b = part;
        for (; b + 24 < nslab; b += 32) {
            s0 += ws[(int64_t)b * n + i];
            s1 += ws[(int64_t)(b + 8) * n + i];
            s2 += ws[(int64_t)(b + 16) * n + i];
            s3 += ws[(int64_t)(b + 24) * n + i];
        }
        for (; b < nslab; b += 8) s0 += ws[(int64_t)b * n + i];
    }
    red[part][e] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (part == 0 && i < n) {
        float t = red[0][e];
#pragma unroll
        for (int q = 1; q < 8; ++q) t += red[q][e];
        dw[i] = t * gscale;
    }
}

// ------------------------------------------------------------------------------------------------ data gradient
struct EWDArgs {
    const unsigned short* dy; const float* w; float* dx;
    int N, Cin, IH, IW, Cout, OH, OW; float gscale;
};

template <int DT, int CP, int K>
__global__ __launch_bounds__(256) void ew_dgrad_kernel(const EWDArgs a) {
    constexpr int NTAP = K == 4 ? 4 : 1;
    __shared__ __attribute__((aligned(16))) float wl[NTAP * 128 * CP];       // [tap][co][ci], ci zero-padded to CP
    const int py = K == 4 ? (int)(blockIdx.y >> 1) : 0, px = K == 4 ? (int)(blockIdx.y & 1) : 0;
    // k4 / s2 / p1: input row iy = 2a + py meets ky = 1 - py + 2 jy at output row a + py - jy (columns alike)
    for (int i = threadIdx.x; i < NTAP * a.Cout * CP; i += 256) {
        const int ci = i % CP, r = i / CP, co = r % a.Cout, t = r / a.Cout;
        const int ky = K == 4 ? 1 - py + 2 * (t >> 1) : 0, kx = K == 4 ? 1 - px + 2 * (t & 1) : 0;
        wl[i] = ci < a.Cin ? a.w[(((int64_t)co * a.Cin + ci) * K + ky) * K + kx] : 0.f;
    }
    __syncthreads();
    const int qh = K == 4 ? (a.IH - py + 1) >> 1 : a.IH, qw = K == 4 ? (a.IW - px + 1) >> 1 : a.IW;
    const int total = a.N * qh * qw;                       // host guarantees < 2^31
    for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
        const int b = p % qw;
        const int r = p / qw;
        const int aa = r % qh;
        const int n = r / qh;
        float acc[CP];
#pragma unroll
        for (int ci = 0; ci < CP; ++ci) acc[ci] = 0.f;
#pragma unroll
        for (int t = 0; t < NTAP; ++t) {
            const int oy = K == 4 ? aa + py - (t >> 1) : aa, ox = K == 4 ? b + px - (t & 1) : b;
            if ((unsigned)oy >= (unsigned)a.OH || (unsigned)ox >= (unsigned)a.OW) continue;
            const unsigned short* dp = a.dy + (((int64_t)n * a.OH + oy) * a.OW + ox) * a.Cout;
            const float* wt = wl + t * a.Cout * CP;
            for (int c0 = 0; c0 < a.Cout; c0 += 8) {
                float g[8];
                unpack8<DT>(*reinterpret_cast<const uint4*>(dp + c0), g);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float* wp = wt + (c0 + i) * CP;
#pragma unroll
                    for (int ci = 0; ci < CP; ++ci) acc[ci] += g[i] * wp[ci];
                }
            }
        }
        const int iy = K == 4 ? 2 * aa + py : aa, ix = K == 4 ? 2 * b + px : b;
#pragma unroll
        for (int ci = 0; ci < CP; ++ci)
            if (ci < a.Cin) a.dx[(((int64_t)n * a.Cin + ci) * a.IH + iy) * a.IW + ix] = acc[ci] * a.gscale;
    }
}

// k: 4 or 1 when the geometry is one of the two covered, else 0
int ew_geom(int k, int stride, int pad) {
    if (k == 4 && stride == 2 && pad == 1) return 4;
    if (k == 1 && stride == 1 && pad == 0) return 1;
    return 0;
}

int ew_check(const char* who, const void* p16, const void* f0, const void* f1, int N, int Cin, int IH, int IW, int Cout, int OH, int OW,
             int k, int stride, int pad, int dtype) {
    GS_CHECK_ARG(p16 && f0 && f1, "%s: null pointer", who);
    GS_CHECK_ARG(((uintptr_t)p16 & 15) == 0 && (((uintptr_t)f0 | (uintptr_t)f1) & 3) == 0,
                 "%s: the 16-bit tensor must be 16-byte aligned, the fp32 tensors 4-byte aligned", who);
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "%s: bad dtype", who);
    GS_CHECK_ARG(N > 0 && IH > 0 && IW > 0 && OH > 0 && OW > 0, "%s: bad dims", who);
    if (Cin < 5 || Cin > 16 || Cout < 8 || Cout > 128 || Cout % 8 != 0 || !ew_geom(k, stride, pad)) return GS_EUNSUPPORTED;
    GS_CHECK_ARG(OH == (IH + 2 * pad - k) / stride + 1 && OW == (IW + 2 * pad - k) / stride + 1 && IH + 2 * pad >= k && IW + 2 * pad >= k,
                 "%s: output size mismatch", who);
    GS_CHECK_ARG((int64_t)N * cdiv(OH, EW_WPH) * cdiv(OW, EW_PW) < 2147483647LL && (int64_t)N * IH * IW < 2147483647LL - 512 * 256,
                 "%s: too many pixels", who);
    return GS_OK;
}

}  // namespace

#define EW_DISPATCH(KERNEL, grid, ...)                                                        \
    do {                                                                                      \
        const int nt_ = cdiv(Cout, 32);                                                       \
        if (dtype == GS_F16) {                                                                \
            if (kg == 4) {                                                                    \
                if (nt_ == 1) KERNEL<GS_F16, 1, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);         \
                else if (nt_ == 2) KERNEL<GS_F16, 2, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);    \
                else if (nt_ == 3) KERNEL<GS_F16, 3, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);    \
                else KERNEL<GS_F16, 4, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);                  \
            } else {                                                                          \
                if (nt_ == 1) KERNEL<GS_F16, 1, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);         \
                else if (nt_ == 2) KERNEL<GS_F16, 2, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);    \
                else if (nt_ == 3) KERNEL<GS_F16, 3, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);    \
                else KERNEL<GS_F16, 4, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);                  \
            }                                                                                 \
        } else {                                                                              \
            if (kg == 4) {                                                                    \
                if (nt_ == 1) KERNEL<GS_BF16, 1, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);        \
                else if (nt_ == 2) KERNEL<GS_BF16, 2, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);   \
                else if (nt_ == 3) KERNEL<GS_BF16, 3, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);   \
                else KERNEL<GS_BF16, 4, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);                 \
            } else {                                                                          \
                if (nt_ == 1) KERNEL<GS_BF16, 1, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);        \
                else if (nt_ == 2) KERNEL<GS_BF16, 2, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);   \
                else if (nt_ == 3) KERNEL<GS_BF16, 3, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);   \
                else KERNEL<GS_BF16, 4, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);                 \
            }                                                                                 \
        }                                                                                     \
    } while (0)

extern "C" int gs_conv_imgwide_fwd(const float* x, const float* w, const float* bias, void* y, int N, int Cin, int IH, int IW, int Cout,
                                   int OH, int OW, int k, int stride, int pad, int act, int dtype, void* stream) {
    int rc = ew_check("gs_conv_imgwide_fwd", y, x, w, N, Cin, IH, IW, Cout, OH, OW, k, stride, pad, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(((uintptr_t)bias & 3) == 0, "gs_conv_imgwide_fwd: misaligned bias");
    if (act != GS_ACT_NONE && act != GS_ACT_LEAKY02) return GS_EUNSUPPORTED;
    const int kg = ew_geom(k, stride, pad);
    const int tiles_x = cdiv(OW, EW_PW), tiles_y = cdiv(OH, EW_FPH);
    EWFArgs a{x, w, bias, (unsigned short*)y, N, Cin, IH, IW, Cout, OH, OW, tiles_x, tiles_y, act};
    hipStream_t s = (hipStream_t)stream;
    const int nb = N * tiles_y * tiles_x;
    EW_DISPATCH(ew_fwd_kernel, nb, a);
    GS_CHECK_LAUNCH("gs_conv_imgwide_fwd");
    return GS_OK;
}

static int ew_wgrad_blocks(int N, int OH, int OW) {
    const int64_t np = (int64_t)N * cdiv(OH, EW_WPH) * cdiv(OW, EW_PW);
    return (int)(np < EW_WGRID ? np : EW_WGRID);
}

extern "C" int64_t gs_conv_imgwide_wgrad_ws_floats(int N, int OH, int OW, int Cin, int Cout, int k) {
    if (N <= 0 || OH <= 0 || OW <= 0 || Cin <= 0 || Cout <= 0 || (k != 4 && k != 1)) return 0;
    return (int64_t)ew_wgrad_blocks(N, OH, OW) * (k == 4 ? EWWGeo<4>::PP : EWWGeo<1>::PP) * Cout * Cin * k * k;
}

extern "C" int gs_conv_imgwide_wgrad(const float* x, const void* dy, float* dw, float* ws, int N, int Cin, int IH, int IW, int Cout,
                                     int OH, int OW, int k, int stride, int pad, float gscale, int dtype, void* stream) {
    int rc = ew_check("gs_conv_imgwide_wgrad", dy, x, dw, N, Cin, IH, IW, Cout, OH, OW, k, stride, pad, dtype);
    if (rc) return rc;
    GS_CHECK_ARG(ws && ((uintptr_t)ws & 3) == 0, "gs_conv_imgwide_wgrad: null or misaligned workspace");
    const int kg = ew_geom(k, stride, pad);
    const int tiles_x = cdiv(OW, EW_PW), tiles_y = cdiv(OH, EW_WPH);
    EWWArgs a{x, (const unsigned short*)dy, ws, N, Cin, IH, IW, Cout, OH, OW, tiles_x, tiles_y, N * tiles_y * tiles_x};
    hipStream_t s = (hipStream_t)stream;
    const int gx = ew_wgrad_blocks(N, OH, OW);
    const dim3 grid(gx, kg == 4 ? cdiv(Cin, EWWGeo<4>::CW) : 1);
    EW_DISPATCH(ew_wgrad_kernel, grid, a);
    const int n = Cout * Cin * k * k;
    ew_slab_sum_kernel<<<cdiv(n, 32), 256, 0, s>>>(ws, gx * (kg == 4 ? EWWGeo<4>::PP : EWWGeo<1>::PP), n, gscale, dw);
    GS_CHECK_LAUNCH("gs_conv_imgwide_wgrad");
    return GS_OK;
}

extern "C" int gs_conv_imgwide_dgrad(const void* dy, const float* w, float* dx, int N, int Cin, int IH, int IW, int Cout, int OH, int OW,
                                     int k, int stride, int pad, float gscale, int dtype, void* stream) {
    int rc = ew_check("gs_conv_imgwide_dgrad", dy, w, dx, N, Cin, IH, IW, Cout, OH, OW, k, stride, pad, dtype);
    if (rc) return rc;
    const int kg = ew_geom(k, stride, pad);
    EWDArgs a{(const unsigned short*)dy, w, dx, N, Cin, IH, IW, Cout, OH, OW, gscale};
    hipStream_t s = (hipStream_t)stream;
    const int64_t per = kg == 4 ? (int64_t)N * ((IH + 1) / 2) * ((IW + 1) / 2) : (int64_t)N * IH * IW;
    const int64_t nb64 = cdiv64(per, 256);
    const dim3 grid((int)(nb64 < 512 ? nb64 : 512), kg == 4 ? 4 : 1);
#define EW_DGRAD(DT)                                                                  \
    do {                                                                              \
        if (kg == 4) {                                                                \
            if (Cin <= 8) ew_dgrad_kernel<DT, 8, 4><<<grid, 256, 0, s>>>(a);          \
            else ew_dgrad_kernel<DT, 16, 4><<<grid, 256, 0, s>>>(a);                  \
        } else {                                                                      \
            if (Cin <= 8) ew_dgrad_kernel<DT, 8, 1><<<grid, 256, 0, s>>>(a);          \
            else ew_dgrad_kernel<DT, 16, 1><<<grid, 256, 0, s>>>(a);                  \
        }                                                                             \
    } while (0)
    if (dtype == GS_F16) EW_DGRAD(GS_F16);
    else EW_DGRAD(GS_BF16);
#undef EW_DGRAD
    GS_CHECK_LAUNCH("gs_conv_imgwide_dgrad");
    return GS_OK;
}
