// The image-side conv of the Pix2Pix networks, for images and for volumes: one kernel family templated on the spatial rank R.
//
//   R = 2  gs_conv_imgwide_*   models_pix2pix/networks.py:640 PatchGAN model.0, :686 PixelDiscriminator net.0, :582 the U-Net generator's
//                              outermost down-conv.  fp32 NCHW image [N,Cin,IH,IW], Cin 5..16 (csrc/direct.hip covers 1..4 and keeps the
//                              whole weight tensor in LDS; at 16 channels x 16 taps x 128 outputs that is 32768 floats, so here it is
//                              tiled), fp32 weights [Cout][Cin][k][k] <-> a dense 16-bit NHWC tensor [N,OH,OW,Cout].
//   R = 3  gs_conv3d_img_*     GenSeg-3D/models/networks.py:829 model.0 of the PatchGAN, :879 net.0 of the PixelDiscriminator, with a 3-D
//                              norm layer.  fp32 NCDHW volume [N,Cin,ID,IH,IW], Cin 1..16, fp32 weights [Cout][Cin][k][k][k] <-> a dense
//                              16-bit tensor [N*OD,OH,OW,Cout] (volumes are stacks of depth slices, as everywhere else).
//
// Cout is any multiple of 8 up to 128, in the two geometries these layers have: k4 / stride 2 / pad 1 and k1 / stride 1 / pad 0.  As in
// csrc/stem_wide.hip the image is NOT rounded to 16 bits and the products are fp32 x fp32 accumulated in fp32 on v_mfma_f32_32x32x2_f32
// (bit-identical to a k-ordered fmaf chain).  An image is a volume of one slice: the args structs are the 3-D ones with ID = OD = 1,
// and the depth coordinate is compiled out of the R = 2 kernels.  A k1 conv is pointwise, so it is rank-free: the 3-D entry points fold
// its depth into the rows ([N,Cin,ID*IH,IW] -> [N,OD*OH,OW,Cout] is the same memory) and launch the same k1 kernels as the 2-D ones.
// ImgGeo<K, R> derives everything else from "64 taps per forward K chunk", "128 taps per weight-gradient chunk" and "8192 floats of
// data-gradient weights":
//
//                            taps / channel   halo slices   forward chunk   wgrad chunk   dgrad taps = classes   dgrad LDS chunk
//   k4, R = 2                      16              1          4 channels     8 channels            4              128 channels
//   k4, R = 3                      64              4          1 channel      2 channels            8               64 channels
//   k1                              1              1         16 channels    16 channels            1              128 channels
//
//   forward   one block per 8 x 32 OUTPUT pixels (of one output slice).  Per chunk of input channels it stages the patch's fp32 halo
//             ([slices][18 rows][66 columns] for k4 -- the zeros of the pad come from the bounds test here, once per halo element)
//             and the weight slab [k][Cout tile rows] (row stride 32 NT + 1).  A stride-2 halo row is stored de-interleaved (even
//             columns, then odd columns): the 32 lanes of an MFMA B operand, which are 32 adjacent OUTPUT columns, then read 32 adjacent
//             floats.  A operand = weights (rows = 32 output channels, permuted so that register g of lane half h is channel 16 h + g),
//             B operand = pixels: a lane ends with one pixel and whole 16-byte channel groups.  Wave w owns patch rows 2w, 2w + 1 and
//             every channel tile.  Epilogue: + bias, LeakyReLU(0.2) or none, round once, 16-byte stores.
//   wgrad     dW = gscale * sum over pixels dy (x) x-taps, also on the fp32 MFMA: A = dy (rows = 32 output channels, k = two pixels),
//             B = the image at (pixel, tap) (columns = 32 taps).  k4: grid.y walks chunks of 128 taps = 4 tap tiles, one per wave, each
//             wave over all 128 pixels of a 4 x 32 patch of one slice; k1: grid.y = 1, one tap tile of 16 channels, the four waves take
//             a quarter of the pixels each.  A block walks patches blockIdx.x, + gridDim.x, ... with its accumulators in registers and
//             writes ONE slab per (block, pixel part); a second launch adds the slabs in index order.  No atomics: two runs give equal
//             bits.
//   dgrad     dx fp32 = gscale * conv_transpose(dy, w).  For k4/s2 each input pixel has 2^R taps fixed by its parity class: grid.y = the
//             2^R classes, the block holds that class's taps x a chunk of output channels x Cin weights in LDS (at most 8192 floats;
//             for volumes a second chunk of 64 channels is restaged per pixel batch, an image's one chunk is staged once) and a thread
//             owns one input pixel and all its channels (wave-uniform LDS reads).
#include <type_traits>

#include "common.hpp"

namespace {

constexpr int EI_PW = 32;                         // output columns of a patch (= MFMA columns)
constexpr int EI_FPH = 8, EI_WPH = 4;             // output rows of a forward / weight-gradient patch
constexpr int EI_WGRID = 256;                     // blocks (per channel chunk) of the weight gradient

template <int K, int R>
struct ImgGeo {
    static_assert((K == 4 && (R == 2 || R == 3)) || (K == 1 && R == 2), "k4 on images or volumes; k1 is rank-free and lives at R = 2");
    static constexpr int S = K == 4 ? 2 : 1, P = K == 4 ? 1 : 0;
    static constexpr int KD = (K == 4 && R == 3) ? 4 : 1;                    // depth taps = halo slices of one output slice
    static constexpr int KK = K * K, TAPS = KK * KD;                         // taps per channel: 16 / 64 / 1
    static constexpr int HC = (EI_PW - 1) * S + K;                           // halo columns: 66 / 32
    static constexpr int CC = K == 4 ? 64 / TAPS : 16;                       // input channels per forward chunk
    static constexpr int CW = K == 4 ? 128 / TAPS : 16;                      // input channels per grid.y chunk of the weight gradient
    static constexpr int TT = K == 4 ? 4 : 1;                                // its 32-tap tiles (k1: 16 taps in one tile)
    static constexpr int PP = 4 / TT;                                        // its pixel parts (waves that share a tap tile)
    static constexpr int DTAP = K == 4 ? 1 << R : 1;                         // taps = parity classes of the data gradient
    static constexpr int DCH = 512 / (1 << R);                               // output channels of its LDS weight chunk
    // position of halo column hx in its row: stride 2 stores the even columns first, then the odd ones
    static __device__ __forceinline__ int col(int hx) { return S == 2 ? (hx & 1) * (HC / 2) + (hx >> 1) : hx; }
    // LDS offset of tap t = ([kz,] ky, kx) inside a channel's halo of `slice` floats per depth slice
    static __device__ __forceinline__ int tap_off(int t, int slice) {
        int kz = 0;
        if constexpr (KD > 1) { kz = t / KK; t -= kz * KK; }
        const int ky = t / K;
        return kz * slice + ky * HC + col(t - K * ky);
    }
    // patch t of a [N][OD][tiles_y][tiles_x] grid -> (n, od, ty, tx)
    template <class A>
    static __device__ __forceinline__ void tile(int t, const A& a, int& n, int& od, int& ty, int& tx) {
        tx = t % a.tiles_x; t /= a.tiles_x;
        ty = t % a.tiles_y; t /= a.tiles_y;
        if constexpr (R == 3) { od = t % a.OD; n = t / a.OD; }
        else { od = 0; n = t; }
    }
    // the fp32 halo of `planes` channels from c0 (channels past cc are zeros) whose first element is input (iz0, iy0, ix0): HR rows
    template <int HR, class A>
    static __device__ __forceinline__ void fill_halo(float* halo, const A& a, int planes, int cc, int n, int c0, int iz0, int iy0,
                                                     int ix0) {
        constexpr int SLICE = HR * HC, PLANE = KD * SLICE;
        for (int i = threadIdx.x; i < planes * PLANE; i += 256) {
            const int ci = i / PLANE, r = i - ci * PLANE;
            const int hz = KD > 1 ? r / SLICE : 0, r2 = r - hz * SLICE;
            const int hy = r2 / HC, hx = r2 - hy * HC;
            const int iz = iz0 + hz, iy = iy0 + hy, ix = ix0 + hx;
            float v = 0.f;
            if (ci < cc && (R == 2 || (unsigned)iz < (unsigned)a.ID) && (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW) {
                int64_t row = (int64_t)n * a.Cin + c0 + ci;
                if constexpr (R == 3) row = row * a.ID + iz;
                v = a.x[(row * a.IH + iy) * a.IW + ix];
            }
            halo[ci * PLANE + hz * SLICE + hy * HC + col(hx)] = v;
        }
    }
};

// ------------------------------------------------------------------------------------------------ forward
struct ImgFArgs {
    const float* x; const float* w; const float* bias; unsigned short* y;
    int N, Cin, ID, IH, IW, Cout, OD, OH, OW, tiles_x, tiles_y, act;
};

template <int DT, int NT, int K, int R>
__global__ __launch_bounds__(256) void img_fwd_kernel(const ImgFArgs a) {
    using G = ImgGeo<K, R>;
    constexpr int S = G::S, TAPS = G::TAPS, HC = G::HC, CC = G::CC;
    constexpr int HR = (EI_FPH - 1) * S + K, SLICE = HR * HC, PLANE = G::KD * SLICE;   // [4 x] 18 x 66 / 8 x 32
    constexpr int KC = CC * TAPS;                                            // K of a full chunk: 64 / 16
    constexpr int WS = NT * 32 + 1;
    static_assert((CC * PLANE + KC * WS) * 4 + KC * 4 <= 64 * 1024, "forward LDS");
    __shared__ float lds[CC * PLANE + KC * WS];                              // halo | weight slab [k][A row]
    __shared__ int koff[KC];
    float* const halo = lds;
    float* const wl = lds + CC * PLANE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    int n, od, ty, tx;
    G::tile(blockIdx.x, a, n, od, ty, tx);
    const int ox0 = tx * EI_PW, oy0 = ty * EI_FPH;
    const int ix0 = ox0 * S - G::P, iy0 = oy0 * S - G::P, iz0 = od * S - G::P;
    if (threadIdx.x < KC) {
        const int k = threadIdx.x, ci = k / TAPS;
        koff[k] = ci * PLANE + G::tap_off(k - ci * TAPS, SLICE);
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
        const int kc = cc * TAPS, kcp = (kc + 1) & ~1;
        const int planes = cc + (kc & 1);                  // odd K (k1, odd cc < CC): one zero plane under the zero weight row
        __syncthreads();                                   // the previous chunk has been read
        G::template fill_halo<HR>(halo, a, planes, cc, n, c0, iz0, iy0, ix0);
        for (int i = threadIdx.x; i < NT * 32 * kcp; i += 256) {
            const int co = i / kcp, k = i - co * kcp;
            const float v = (k < kc && co < a.Cout) ? a.w[((int64_t)co * a.Cin + c0) * TAPS + k] : 0.f;
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

    // the lane holds pixel ([od,] oy0 + 2 wave + r, ox0 + li), channels 32 nt + 16 lh + (0..15): two 16-byte groups per tile
    const int ox = ox0 + li;
    int64_t slice = n;
    if constexpr (R == 3) slice = slice * a.OD + od;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + 2 * wave + r;
        if (ox < a.OW && oy < a.OH) {
            const int64_t base = ((slice * a.OH + oy) * a.OW + ox) * a.Cout;
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
struct ImgWArgs {
    const float* x; const unsigned short* dy; float* ws;
    int N, Cin, ID, IH, IW, Cout, OD, OH, OW, tiles_x, tiles_y, npatch;
};

template <int DT, int NT, int K, int R>
__global__ __launch_bounds__(256) void img_wgrad_kernel(const ImgWArgs a) {
    using G = ImgGeo<K, R>;
    constexpr int S = G::S, TAPS = G::TAPS, HC = G::HC;
    constexpr int CW = G::CW, TT = G::TT, PP = G::PP;
    constexpr int HR = (EI_WPH - 1) * S + K, SLICE = HR * HC, PLANE = G::KD * SLICE;   // [4 x] 10 x 66 / 4 x 32
    constexpr int NPIX = EI_WPH * EI_PW;                                     // 128
    constexpr int RS = NT * 32 + 8;                                          // dy row stride (16-bit elements, 16-byte multiple)
    static_assert(CW * PLANE * 4 + NPIX * RS * 2 <= 64 * 1024, "weight-gradient LDS");
    __shared__ float halo[CW * PLANE];
    __shared__ __attribute__((aligned(16))) unsigned short dyl[NPIX * RS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int tt = wave % TT, pp = wave / TT;
    const int c0 = blockIdx.y * CW;
    const int cc = a.Cin - c0 < CW ? a.Cin - c0 : CW;
    const int tap = tt * 32 + li;                          // the lane's B column: tap (ci, [kz,] ky, kx) of the chunk
    const bool tap_ok = tap < cc * TAPS;
    int tapoff = 0;                                        // (a dead column reads plane 0: finite values, never stored)
    if (tap_ok) {
        const int ci = tap / TAPS;
        tapoff = ci * PLANE + G::tap_off(tap - ci * TAPS, SLICE);
    }
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[nt][g] = 0.f;
    const int ngrp = a.Cout >> 3;

    for (int pt = blockIdx.x; pt < a.npatch; pt += gridDim.x) {
        int n, od, ty, tx;
        G::tile(pt, a, n, od, ty, tx);
        const int ox0 = tx * EI_PW, oy0 = ty * EI_WPH;
        const int ix0 = ox0 * S - G::P, iy0 = oy0 * S - G::P, iz0 = od * S - G::P;
        int64_t slice = n;
        if constexpr (R == 3) slice = slice * a.OD + od;
        __syncthreads();                                   // the previous patch has been read
        G::template fill_halo<HR>(halo, a, CW, cc, n, c0, iz0, iy0, ix0);
        for (int i = threadIdx.x; i < NPIX * (NT * 4); i += 256) {           // every 16-byte group of the NT * 32 channel columns
            const int p = i / (NT * 4), g = i - p * (NT * 4);
            const int oy = oy0 + (p >> 5), ox = ox0 + (p & 31);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);                            // pixels outside the slice and channels past Cout: zeros
            if (g < ngrp && oy < a.OH && ox < a.OW)
                v = *reinterpret_cast<const uint4*>(a.dy + ((slice * a.OH + oy) * a.OW + ox) * a.Cout + g * 8);
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
    const int T = a.Cin * TAPS;
    float* const slab = a.ws + ((int64_t)blockIdx.x * PP + pp) * a.Cout * T + c0 * TAPS + tap;
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
__global__ __launch_bounds__(256) void img_slab_sum_kernel(const float* ws, int nslab, int n, float gscale, float* dw) {
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
struct ImgDArgs {
    const unsigned short* dy; const float* w; float* dx;
    int N, Cin, ID, IH, IW, Cout, OD, OH, OW; float gscale;
};

// the data gradient's LDS weights [tap][co of the chunk][ci] for output channels co0 .. co0 + cn of parity class (pz, py, px)
template <int CP, int K, int R>
__device__ __forceinline__ void img_dgrad_stage(float* wl, const ImgDArgs& a, int pz, int py, int px, int co0, int cn) {
    using G = ImgGeo<K, R>;
    for (int i = threadIdx.x; i < G::DTAP * cn * CP; i += 256) {
        const int ci = i % CP, q = i / CP, co = q % cn, t = q / cn;
        int kt = 0;                                        // the weight's tap ([kz,] ky, kx)
        if constexpr (K == 4) {
            kt = (1 - py + 2 * ((t >> 1) & 1)) * K + 1 - px + 2 * (t & 1);
            if constexpr (R == 3) kt += (1 - pz + 2 * (t >> 2)) * K * K;
        }
        wl[(t * G::DCH + co) * CP + ci] = ci < a.Cin ? a.w[((int64_t)(co0 + co) * a.Cin + ci) * G::TAPS + kt] : 0.f;
    }
    __syncthreads();
}

template <int DT, int CP, int K, int R>
__global__ __launch_bounds__(256) void img_dgrad_kernel(const ImgDArgs a) {
    using G = ImgGeo<K, R>;
    constexpr int NTAP = G::DTAP, DCH = G::DCH;
    constexpr bool ONE = DCH >= 128;                       // Cout <= 128 is always one chunk
    __shared__ __attribute__((aligned(16))) float wl[NTAP * DCH * CP];       // [tap][co of the chunk][ci], ci zero-padded to CP
    // class bits and tap bits, x fastest: k4 / s2 / p1: input row iy = 2a + py meets ky = 1 - py + 2 jy at output row a + py - jy
    // (slices and columns alike)
    const int cls = K == 4 ? (int)blockIdx.y : 0;
    const int px = cls & 1, py = (cls >> 1) & 1, pz = R == 3 ? cls >> 2 : 0;
    const int qd = R == 3 ? (a.ID - pz + 1) >> 1 : 1, qh = K == 4 ? (a.IH - py + 1) >> 1 : a.IH,
              qw = K == 4 ? (a.IW - px + 1) >> 1 : a.IW;
    const int total = a.N * qd * qh * qw;                  // host guarantees < 2^31 - the grid's stride
    const int nck = ONE ? 1 : (a.Cout + DCH - 1) / DCH;
    // ONE: staged here, then each thread walks its own pixels p0.  Else the block walks batches of 256 pixels from p0 together (a thread
    // past the end is not live but keeps the barriers): one chunk is staged at the first batch, two are restaged at every batch
    if constexpr (ONE) img_dgrad_stage<CP, K, R>(wl, a, pz, py, px, 0, a.Cout);
    bool staged = ONE;
    for (int p0 = blockIdx.x * 256 + (ONE ? (int)threadIdx.x : 0); p0 < total; p0 += gridDim.x * 256) {
        const int p = ONE ? p0 : p0 + (int)threadIdx.x;
        const bool live = ONE || p < total;
        const int b = p % qw;
        int r = p / qw;
        const int aa = r % qh; r /= qh;
        int ad = 0, n = r;
        if constexpr (R == 3) { ad = r % qd; n = r / qd; }
        float acc[CP];
#pragma unroll
        for (int ci = 0; ci < CP; ++ci) acc[ci] = 0.f;
        for (int ck = 0; ck < nck; ++ck) {
            const int co0 = ck * DCH;
            const int cn = ONE ? a.Cout : a.Cout - co0 < DCH ? a.Cout - co0 : DCH;
            if (nck > 1 || !staged) {                      // block-uniform
                __syncthreads();
                img_dgrad_stage<CP, K, R>(wl, a, pz, py, px, co0, cn);
                staged = true;
            }
            if (!live) continue;
#pragma unroll
            for (int t = 0; t < NTAP; ++t) {
                const int oy = K == 4 ? aa + py - ((t >> 1) & 1) : aa, ox = K == 4 ? b + px - (t & 1) : b;
                if ((unsigned)oy >= (unsigned)a.OH || (unsigned)ox >= (unsigned)a.OW) continue;
                int64_t slice = n;
                if constexpr (R == 3) {
                    const int oz = ad + pz - (t >> 2);
                    if ((unsigned)oz >= (unsigned)a.OD) continue;
                    slice = slice * a.OD + oz;
                }
                const unsigned short* dp = a.dy + ((slice * a.OH + oy) * a.OW + ox) * a.Cout + co0;
                const float* wt = wl + t * DCH * CP;
                for (int c = 0; c < cn; c += 8) {
                    float g[8];
                    unpack8<DT>(*reinterpret_cast<const uint4*>(dp + c), g);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float* wp = wt + (c + i) * CP;
#pragma unroll
                        for (int ci = 0; ci < CP; ++ci) acc[ci] += g[i] * wp[ci];
                    }
                }
            }
        }
        if (live) {
            const int iy = K == 4 ? 2 * aa + py : aa, ix = K == 4 ? 2 * b + px : b;
#pragma unroll
            for (int ci = 0; ci < CP; ++ci)
                if (ci < a.Cin) {
                    int64_t row = (int64_t)n * a.Cin + ci;
                    if constexpr (R == 3) row = row * a.ID + 2 * ad + pz;
                    a.dx[(row * a.IH + iy) * a.IW + ix] = acc[ci] * a.gscale;
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// k: 4 or 1 when the geometry is one of the two covered, else 0
int img_geom(int k, int stride, int pad) {
    if (k == 4 && stride == 2 && pad == 1) return 4;
    if (k == 1 && stride == 1 && pad == 0) return 1;
    return 0;
}

// the dims as the kernels see them: an image has ID = OD = 1; a k1 conv is pointwise: its depth is folded into the rows
struct ImgDims { int ID, IH, IW, OD, OH, OW; };

// rank 2: Cin from cin_min = 5 (csrc/direct.hip owns 1..4); rank 3: from 1
int img_check(const char* who, int rank, int cin_min, const void* p16, const void* f0, const void* f1, int N, int Cin, int Cout, int k,
              int stride, int pad, int dtype, ImgDims& d) {
    GS_CHECK_ARG(p16 && f0 && f1, "%s: null pointer", who);
    GS_CHECK_ARG(((uintptr_t)p16 & 15) == 0 && (((uintptr_t)f0 | (uintptr_t)f1) & 3) == 0,
                 "%s: the 16-bit tensor must be 16-byte aligned, the fp32 tensors 4-byte aligned", who);
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "%s: bad dtype", who);
    GS_CHECK_ARG(N > 0 && d.ID > 0 && d.IH > 0 && d.IW > 0 && d.OD > 0 && d.OH > 0 && d.OW > 0, "%s: bad dims", who);
    if (Cin < cin_min || Cin > 16 || Cout < 8 || Cout > 128 || Cout % 8 != 0 || !img_geom(k, stride, pad)) return GS_EUNSUPPORTED;
    const int e = 2 * pad - k;
    GS_CHECK_ARG((rank == 2 || (d.ID + e >= 0 && d.OD == (d.ID + e) / stride + 1)) && d.IH + e >= 0 && d.IW + e >= 0 &&
                     d.OH == (d.IH + e) / stride + 1 && d.OW == (d.IW + e) / stride + 1,
                 "%s: output size mismatch", who);
    GS_CHECK_ARG((int64_t)N * d.OD * cdiv(d.OH, EI_WPH) * cdiv(d.OW, EI_PW) < 2147483647LL &&
                     (int64_t)N * d.ID * d.IH * d.IW < 2147483647LL - 512 * 256,
                 "%s: too many %s", who, rank == 2 ? "pixels" : "voxels");
    if (k == 1) {
        d.IH *= d.ID; d.OH *= d.OD;
        d.ID = d.OD = 1;
    }
    return GS_OK;
}

template <int V> using Int = std::integral_constant<int, V>;

// f(DT, SEL, K, R) as compile-time constants: dtype x sel 1..4 x (k4 rank 2 | k4 rank 3 | k1).  sel is NT, or CP = 1 << sel
template <class F>
void img_dispatch(int dtype, int sel, int kg, int rank, F f) {
    auto geom = [&](auto dt, auto sl) {
        if (kg == 1) f(dt, sl, Int<1>{}, Int<2>{});
        else if (rank == 2) f(dt, sl, Int<4>{}, Int<2>{});
        else f(dt, sl, Int<4>{}, Int<3>{});
    };
    auto nsel = [&](auto dt) {
        if (sel == 1) geom(dt, Int<1>{});
        else if (sel == 2) geom(dt, Int<2>{});
        else if (sel == 3) geom(dt, Int<3>{});
        else geom(dt, Int<4>{});
    };
    if (dtype == GS_F16) nsel(Int<GS_F16>{});
    else nsel(Int<GS_BF16>{});
}

int img_wgrad_blocks(int N, const ImgDims& d) {
    const int64_t np = (int64_t)N * d.OD * cdiv(d.OH, EI_WPH) * cdiv(d.OW, EI_PW);
    return (int)(np < EI_WGRID ? np : EI_WGRID);
}

// what the host needs of ImgGeo<K, R>: taps per channel, the weight gradient's channel chunk and pixel parts, the data gradient's classes
struct ImgHostGeo { int taps, cw, pp, dtap; };

template <int K, int R>
constexpr ImgHostGeo img_host_geo() { return {ImgGeo<K, R>::TAPS, ImgGeo<K, R>::CW, ImgGeo<K, R>::PP, ImgGeo<K, R>::DTAP}; }

ImgHostGeo img_host_geo(int kg, int rank) {
    return kg == 1 ? img_host_geo<1, 2>() : rank == 2 ? img_host_geo<4, 2>() : img_host_geo<4, 3>();
}

int img_fwd(const char* who, int rank, int cin_min, const float* x, const float* w, const float* bias, void* y, int N, int Cin,
            ImgDims d, int Cout, int k, int stride, int pad, int act, int dtype, void* stream) {
    int rc = img_check(who, rank, cin_min, y, x, w, N, Cin, Cout, k, stride, pad, dtype, d);
    if (rc) return rc;
    GS_CHECK_ARG(((uintptr_t)bias & 3) == 0, "%s: misaligned bias", who);
    if (act != GS_ACT_NONE && act != GS_ACT_LEAKY02) return GS_EUNSUPPORTED;
    const int tiles_x = cdiv(d.OW, EI_PW), tiles_y = cdiv(d.OH, EI_FPH);
    const ImgFArgs a{x, w, bias, (unsigned short*)y, N, Cin, d.ID, d.IH, d.IW, Cout, d.OD, d.OH, d.OW, tiles_x, tiles_y, act};
    hipStream_t s = (hipStream_t)stream;
    const int nb = N * d.OD * tiles_y * tiles_x;
    img_dispatch(dtype, cdiv(Cout, 32), img_geom(k, stride, pad), rank, [&](auto dt, auto nt, auto kk, auto r) {
        img_fwd_kernel<dt(), nt(), kk(), r()><<<nb, 256, 0, s>>>(a);
    });
    GS_CHECK_LAUNCH(who);
    return GS_OK;
}

int64_t img_wgrad_ws_floats(int rank, int N, int OD, int OH, int OW, int Cin, int Cout, int k) {
    if (N <= 0 || OD <= 0 || OH <= 0 || OW <= 0 || Cin <= 0 || Cout <= 0 || (k != 4 && k != 1)) return 0;
    if (rank == 3 && (int64_t)N * OD * OH >= 2147483647LL) return 0;
    ImgDims d{1, 1, 1, OD, OH, OW};
    if (k == 1) { d.OH *= OD; d.OD = 1; }
    const ImgHostGeo g = img_host_geo(k, rank);
    return (int64_t)img_wgrad_blocks(N, d) * g.pp * Cout * Cin * g.taps;
}

int img_wgrad(const char* who, int rank, int cin_min, const float* x, const void* dy, float* dw, float* ws, int N, int Cin, ImgDims d,
              int Cout, int k, int stride, int pad, float gscale, int dtype, void* stream) {
    int rc = img_check(who, rank, cin_min, dy, x, dw, N, Cin, Cout, k, stride, pad, dtype, d);
    if (rc) return rc;
    GS_CHECK_ARG(ws && ((uintptr_t)ws & 3) == 0, "%s: null or misaligned workspace", who);
    const int kg = img_geom(k, stride, pad);
    const ImgHostGeo g = img_host_geo(kg, rank);
    const int tiles_x = cdiv(d.OW, EI_PW), tiles_y = cdiv(d.OH, EI_WPH);
    const ImgWArgs a{x, (const unsigned short*)dy, ws, N, Cin, d.ID, d.IH, d.IW, Cout, d.OD, d.OH, d.OW, tiles_x, tiles_y,
                     N * d.OD * tiles_y * tiles_x};
    hipStream_t s = (hipStream_t)stream;
    const int gx = img_wgrad_blocks(N, d);
    const dim3 grid(gx, cdiv(Cin, g.cw));
    img_dispatch(dtype, cdiv(Cout, 32), kg, rank, [&](auto dt, auto nt, auto kk, auto r) {
        img_wgrad_kernel<dt(), nt(), kk(), r()><<<grid, 256, 0, s>>>(a);
    });
    const int n = Cout * Cin * g.taps;
    img_slab_sum_kernel<<<cdiv(n, 32), 256, 0, s>>>(ws, gx * g.pp, n, gscale, dw);
    GS_CHECK_LAUNCH(who);
    return GS_OK;
}

int img_dgrad(const char* who, int rank, int cin_min, const void* dy, const float* w, float* dx, int N, int Cin, ImgDims d, int Cout,
              int k, int stride, int pad, float gscale, int dtype, void* stream) {
    int rc = img_check(who, rank, cin_min, dy, w, dx, N, Cin, Cout, k, stride, pad, dtype, d);
    if (rc) return rc;
    const int kg = img_geom(k, stride, pad);
    const ImgDArgs a{(const unsigned short*)dy, w, dx, N, Cin, d.ID, d.IH, d.IW, Cout, d.OD, d.OH, d.OW, gscale};
    hipStream_t s = (hipStream_t)stream;
    const int64_t per = kg == 4 ? (int64_t)N * ((d.ID + 1) / 2) * ((d.IH + 1) / 2) * ((d.IW + 1) / 2) : (int64_t)N * d.ID * d.IH * d.IW;
    const int64_t nb64 = cdiv64(per, 256);
    const dim3 grid((int)(nb64 < 512 ? nb64 : 512), img_host_geo(kg, rank).dtap);
    // channels padded to CP = 1 << sel; an image has at least 5 (and keeps CP 8 at k1, as before)
    const int sel = Cin <= 2 && rank == 3 ? 1 : Cin <= 4 && rank == 3 ? 2 : Cin <= 8 ? 3 : 4;
    img_dispatch(dtype, sel, kg, rank, [&](auto dt, auto sl, auto kk, auto r) {
        constexpr int CP = 1 << sl();
        if constexpr (CP >= 8 || kk() == 1 || r() == 3) img_dgrad_kernel<dt(), CP, kk(), r()><<<grid, 256, 0, s>>>(a);
    });
    GS_CHECK_LAUNCH(who);
    return GS_OK;
}

}  // namespace

extern "C" int gs_conv_imgwide_fwd(const float* x, const float* w, const float* bias, void* y, int N, int Cin, int IH, int IW, int Cout,
                                   int OH, int OW, int k, int stride, int pad, int act, int dtype, void* stream) {
    return img_fwd("gs_conv_imgwide_fwd", 2, 5, x, w, bias, y, N, Cin, {1, IH, IW, 1, OH, OW}, Cout, k, stride, pad, act, dtype, stream);
}

extern "C" int64_t gs_conv_imgwide_wgrad_ws_floats(int N, int OH, int OW, int Cin, int Cout, int k) {
    return img_wgrad_ws_floats(2, N, 1, OH, OW, Cin, Cout, k);
}

extern "C" int gs_conv_imgwide_wgrad(const float* x, const void* dy, float* dw, float* ws, int N, int Cin, int IH, int IW, int Cout,
                                     int OH, int OW, int k, int stride, int pad, float gscale, int dtype, void* stream) {
    return img_wgrad("gs_conv_imgwide_wgrad", 2, 5, x, dy, dw, ws, N, Cin, {1, IH, IW, 1, OH, OW}, Cout, k, stride, pad, gscale, dtype,
                     stream);
}

extern "C" int gs_conv_imgwide_dgrad(const void* dy, const float* w, float* dx, int N, int Cin, int IH, int IW, int Cout, int OH, int OW,
                                     int k, int stride, int pad, float gscale, int dtype, void* stream) {
    return img_dgrad("gs_conv_imgwide_dgrad", 2, 5, dy, w, dx, N, Cin, {1, IH, IW, 1, OH, OW}, Cout, k, stride, pad, gscale, dtype,
                     stream);
}

extern "C" int gs_conv3d_img_fwd(const float* x, const float* w, const float* bias, void* y, int N, int Cin, int ID, int IH, int IW,
                                 int Cout, int OD, int OH, int OW, int k, int stride, int pad, int act, int dtype, void* stream) {
    return img_fwd("gs_conv3d_img_fwd", 3, 1, x, w, bias, y, N, Cin, {ID, IH, IW, OD, OH, OW}, Cout, k, stride, pad, act, dtype, stream);
}

extern "C" int64_t gs_conv3d_img_wgrad_ws_floats(int N, int OD, int OH, int OW, int Cin, int Cout, int k) {
    return img_wgrad_ws_floats(3, N, OD, OH, OW, Cin, Cout, k);
}

extern "C" int gs_conv3d_img_wgrad(const float* x, const void* dy, float* dw, float* ws, int N, int Cin, int ID, int IH, int IW, int Cout,
                                   int OD, int OH, int OW, int k, int stride, int pad, float gscale, int dtype, void* stream) {
    return img_wgrad("gs_conv3d_img_wgrad", 3, 1, x, dy, dw, ws, N, Cin, {ID, IH, IW, OD, OH, OW}, Cout, k, stride, pad, gscale, dtype,
                     stream);
}

extern "C" int gs_conv3d_img_dgrad(const void* dy, const float* w, float* dx, int N, int Cin, int ID, int IH, int IW, int Cout, int OD,
                                   int OH, int OW, int k, int stride, int pad, float gscale, int dtype, void* stream) {
    return img_dgrad("gs_conv3d_img_dgrad", 3, 1, dy, w, dx, N, Cin, {ID, IH, IW, OD, OH, OW}, Cout, k, stride, pad, gscale, dtype,
                     stream);
}
