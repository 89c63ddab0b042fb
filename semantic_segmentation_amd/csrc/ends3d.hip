// The two ends of the 3-D Pix2Pix discriminators (GenSeg-3D/models/networks.py:806-890 with a 3-D norm layer: NLayerDiscriminator
// and PixelDiscriminator hold nn.Conv3d leaves).  Volumes are stacks of depth slices, as everywhere else: [N*D, H, W, C] in 16 bits.
//
// IMAGE SIDE (model.0 of the PatchGAN, :829; net.0 of the PixelDiscriminator, :879): fp32 NCDHW volume [N,Cin,ID,IH,IW], Cin 1..16,
// and fp32 weights in the reference layout [Cout][Cin][k][k][k] <-> a dense 16-bit tensor [N*OD,OH,OW,Cout], Cout any multiple of 8
// up to 128, in the two geometries these layers have: k4 / stride 2 / pad 1 and k1 / stride 1 / pad 0.  This is csrc/ends_wide.hip
// with a depth axis (read that file's header first): the volume is NOT rounded to 16 bits, the products are fp32 x fp32 accumulated
// in fp32 on v_mfma_f32_32x32x2_f32 (bit-identical to a k-ordered fmaf chain).  A k1 conv is pointwise, so the entry points fold its
// depth into the rows ([N,Cin,ID*IH,IW] -> [N,OD*OH,OW,Cout] is the same memory) and the k1 kernels run with one depth slice.
//
//   gs_conv3d_img_fwd    one block per 8 x 32 OUTPUT voxels of one output slice.  k4: ONE input channel per chunk -- its 4 x 4 x 4 taps
//                        are a K of 64 -- with the patch's fp32 halo [4 slices][18 rows][66 columns] (the zeros of the pad come from
//                        the bounds test, once per halo element; a stride-2 halo row is stored de-interleaved, even columns then odd
//                        ones, so that the 32 lanes of a B operand read 32 adjacent floats) and the weight slab [k][Cout tile rows]
//                        (row stride 32 NT + 1) in LDS.  k1: 16 channels per chunk.  A operand = weights, B operand = voxels; wave w
//                        owns patch rows 2w, 2w + 1 and every channel tile.  Epilogue: + bias, LeakyReLU(0.2) or none, round once,
//                        16-byte stores.
//   gs_conv3d_img_wgrad  dW = gscale * sum over voxels dy (x) x-taps: A = dy (rows = 32 output channels, k = two voxels), B = the
//                        volume at (voxel, tap) (columns = 32 taps).  k4: grid.y walks chunks of 2 channels = 128 taps = 4 tap tiles,
//                        one per wave, each wave over all 128 voxels of a 4 x 32 patch of one slice; k1: one tap tile of 16 channels,
//                        the four waves take a quarter of the voxels each.  A block walks patches blockIdx.x, + gridDim.x, ... with
//                        its accumulators in registers and writes ONE slab per (block, voxel part); a second launch adds the slabs in
//                        index order.  No atomics: two runs give equal bits.
//   gs_conv3d_img_dgrad  dx fp32 NCDHW = gscale * conv_transpose3d(dy, w).  k4/s2: each input voxel has 2 x 2 x 2 taps fixed by its
//                        parity class: grid.y = the 8 classes; the block holds the class's 8 taps x 64 output channels x Cin weights
//                        in LDS (at most 8192 floats; a second chunk of 64 channels is restaged) and a thread owns one input voxel
//                        and all its channels (wave-uniform LDS reads).
//
// ONE-CHANNEL HEAD (the last conv of both: Conv3d(C, 1, k4, s1, p1), :850, and Conv3d(C, 1, k1), :884): 16-bit [N*D,H,W,Cin], Cin a
// multiple of 8 up to 1024, fp32 weights [1][Cin][k][k][k] -> fp32 logits [N,1,OD,OH,OW]; the contract of gs_conv_smallcout_fwd /
// _bwd.  The output volume is tiny (6^3 at a 64^3 crop) under a K of up to 65536, so the k4 forward is a REDUCTION: one block per
// logit, the 256 threads take (tap, 8-channel group) items, taps fastest (adjacent lanes read adjacent weights), and the block sum
// has a fixed order.  k1: 8 lanes per voxel.  Backward: dz 16-bit = sum over taps dl * w, rounded once (k4: grid.y = the 8-channel
// group, so its 512 weights are wave-uniform; k1: a thread per (voxel, group)); dw and db += gscale * sums, through per-part slabs
// (a thread owns one (tap, group) item = 8 weights and walks the part's logits) added in part order by a second launch.
#include "common.hpp"

namespace {

constexpr int E3_PW = 32;                         // output columns of a patch (= MFMA columns)
constexpr int E3_FPH = 8, E3_WPH = 4;             // output rows of a forward / weight-gradient patch
constexpr int E3_WGRID = 256;                     // blocks (per channel chunk) of the weight gradient

template <int K>
struct E3Geo {
    static constexpr int S = K == 4 ? 2 : 1, P = K == 4 ? 1 : 0, KK = K * K, KKK = K * K * K;
    static constexpr int HC = (E3_PW - 1) * S + K;                           // halo columns: 66 / 32
    static constexpr int HD = K;                                             // halo slices of one output slice: 4 / 1
    // position of halo column hx in its row: stride 2 stores the even columns first, then the odd ones
    static __device__ __forceinline__ int col(int hx) { return S == 2 ? (hx & 1) * (HC / 2) + (hx >> 1) : hx; }
    // LDS offset of tap t = (kz, ky, kx) inside a channel's halo of `slice` floats per depth slice
    static __device__ __forceinline__ int tap_off(int t, int slice) {
        const int kz = t / KK, r = t - kz * KK, ky = r / K;
        return kz * slice + ky * HC + col(r - K * ky);
    }
};

// ------------------------------------------------------------------------------------------------ forward
struct E3FArgs {
    const float* x; const float* w; const float* bias; unsigned short* y;
    int N, Cin, ID, IH, IW, Cout, OD, OH, OW, tiles_x, tiles_y, act;
};

template <int DT, int NT, int K>
__global__ __launch_bounds__(256) void e3_fwd_kernel(const E3FArgs a) {
    using G = E3Geo<K>;
    constexpr int S = G::S, KKK = G::KKK, HC = G::HC, HD = G::HD;
    constexpr int CC = K == 4 ? 1 : 16;                                      // input channels per chunk
    constexpr int HR = (E3_FPH - 1) * S + K, SLICE = HR * HC, PLANE = HD * SLICE;   // 4 x 18 x 66 / 1 x 8 x 32
    constexpr int KC = CC * KKK;                                             // K of a full chunk: 64 / 16
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
    const int ty = t % a.tiles_y; t /= a.tiles_y;
    const int od = t % a.OD;
    const int n = t / a.OD;
    const int ox0 = tx * E3_PW, oy0 = ty * E3_FPH;
    const int ix0 = ox0 * S - G::P, iy0 = oy0 * S - G::P, iz0 = od * S - G::P;
    if (threadIdx.x < KC) {
        const int k = threadIdx.x, ci = k / KKK;
        koff[k] = ci * PLANE + G::tap_off(k - ci * KKK, SLICE);
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
        const int kc = cc * KKK, kcp = (kc + 1) & ~1;
        const int planes = cc + (kc & 1);                  // odd K (k1, odd cc < CC): one zero plane under the zero weight row
        __syncthreads();                                   // the previous chunk has been read
        for (int i = threadIdx.x; i < planes * PLANE; i += 256) {
            const int ci = i / PLANE, r = i - ci * PLANE;
            const int hz = r / SLICE, r2 = r - hz * SLICE;
            const int hy = r2 / HC, hx = r2 - hy * HC;
            const int iz = iz0 + hz, iy = iy0 + hy, ix = ix0 + hx;
            float v = 0.f;
            if (ci < cc && (unsigned)iz < (unsigned)a.ID && (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW)
                v = a.x[((((int64_t)n * a.Cin + c0 + ci) * a.ID + iz) * a.IH + iy) * a.IW + ix];
            halo[ci * PLANE + hz * SLICE + hy * HC + G::col(hx)] = v;
        }
        for (int i = threadIdx.x; i < NT * 32 * kcp; i += 256) {
            const int co = i / kcp, k = i - co * kcp;
            const float v = (k < kc && co < a.Cout) ? a.w[((int64_t)co * a.Cin + c0) * KKK + k] : 0.f;
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

    // the lane holds voxel (od, oy0 + 2 wave + r, ox0 + li), channels 32 nt + 16 lh + (0..15): two 16-byte groups per tile
    const int ox = ox0 + li;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + 2 * wave + r;
        if (ox < a.OW && oy < a.OH) {
            const int64_t base = ((((int64_t)n * a.OD + od) * a.OH + oy) * a.OW + ox) * a.Cout;
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
struct E3WArgs {
    const float* x; const unsigned short* dy; float* ws;
    int N, Cin, ID, IH, IW, Cout, OD, OH, OW, tiles_x, tiles_y, npatch;
};

template <int K> struct E3WGeo {
    static constexpr int CW = K == 4 ? 2 : 16;            // volume channels per grid.y chunk
    static constexpr int TT = K == 4 ? 4 : 1;             // 32-tap tiles per chunk (k4: 2 channels x 64 taps; k1: 16 taps in one tile)
    static constexpr int PP = 4 / TT;                     // voxel parts (waves that share a tap tile)
};

template <int DT, int NT, int K>
__global__ __launch_bounds__(256) void e3_wgrad_kernel(const E3WArgs a) {
    using G = E3Geo<K>;
    using GW = E3WGeo<K>;
    constexpr int S = G::S, KKK = G::KKK, HC = G::HC, HD = G::HD;
    constexpr int CW = GW::CW, TT = GW::TT, PP = GW::PP;
    constexpr int HR = (E3_WPH - 1) * S + K, SLICE = HR * HC, PLANE = HD * SLICE;   // 4 x 10 x 66 / 1 x 4 x 32
    constexpr int NPIX = E3_WPH * E3_PW;                                     // 128
    constexpr int RS = NT * 32 + 8;                                          // dy row stride (16-bit elements, 16-byte multiple)
    static_assert(CW * PLANE * 4 + NPIX * RS * 2 <= 64 * 1024, "weight-gradient LDS");
    __shared__ float halo[CW * PLANE];
    __shared__ __attribute__((aligned(16))) unsigned short dyl[NPIX * RS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int tt = wave % TT, pp = wave / TT;
    const int c0 = blockIdx.y * CW;
    const int cc = a.Cin - c0 < CW ? a.Cin - c0 : CW;
    const int tap = tt * 32 + li;                          // the lane's B column: tap (ci, kz, ky, kx) of the chunk
    const bool tap_ok = tap < cc * KKK;
    int tapoff = 0;                                        // (a dead column reads plane 0: finite values, never stored)
    if (tap_ok) {
        const int ci = tap / KKK;
        tapoff = ci * PLANE + G::tap_off(tap - ci * KKK, SLICE);
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
        const int ty = t % a.tiles_y; t /= a.tiles_y;
        const int od = t % a.OD;
        const int n = t / a.OD;
        const int ox0 = tx * E3_PW, oy0 = ty * E3_WPH;
        const int ix0 = ox0 * S - G::P, iy0 = oy0 * S - G::P, iz0 = od * S - G::P;
        __syncthreads();                                   // the previous patch has been read
        for (int i = threadIdx.x; i < CW * PLANE; i += 256) {
            const int ci = i / PLANE, r = i - ci * PLANE;
            const int hz = r / SLICE, r2 = r - hz * SLICE;
            const int hy = r2 / HC, hx = r2 - hy * HC;
            const int iz = iz0 + hz, iy = iy0 + hy, ix = ix0 + hx;
            float v = 0.f;
            if (ci < cc && (unsigned)iz < (unsigned)a.ID && (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW)
                v = a.x[((((int64_t)n * a.Cin + c0 + ci) * a.ID + iz) * a.IH + iy) * a.IW + ix];
            halo[ci * PLANE + hz * SLICE + hy * HC + G::col(hx)] = v;
        }
        for (int i = threadIdx.x; i < NPIX * (NT * 4); i += 256) {           // every 16-byte group of the NT * 32 channel columns
            const int p = i / (NT * 4), g = i - p * (NT * 4);
            const int oy = oy0 + (p >> 5), ox = ox0 + (p & 31);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);                            // voxels outside the slice and channels past Cout: zeros
            if (g < ngrp && oy < a.OH && ox < a.OW)
                v = *reinterpret_cast<const uint4*>(a.dy + ((((int64_t)n * a.OD + od) * a.OH + oy) * a.OW + ox) * a.Cout + g * 8);
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
    const int T = a.Cin * KKK;
    float* const slab = a.ws + ((int64_t)blockIdx.x * PP + pp) * a.Cout * T + c0 * KKK + tap;
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
__global__ __launch_bounds__(256) void e3_slab_sum_kernel(const float* ws, int nslab, int n, float gscale, float* dw) {
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
struct E3DArgs {
    const unsigned short* dy; const float* w; float* dx;
    int N, Cin, ID, IH, IW, Cout, OD, OH, OW; float gscale;
};

constexpr int E3_DCH = 64;                                 // output channels of the data gradient's LDS weight chunk

template <int DT, int CP, int K>
__global__ __launch_bounds__(256) void e3_dgrad_kernel(const E3DArgs a) {
    constexpr int NTAP = K == 4 ? 8 : 1, KKK = K * K * K;
    __shared__ __attribute__((aligned(16))) float wl[NTAP * E3_DCH * CP];    // [tap][co of the chunk][ci], ci zero-padded to CP
    const int cls = K == 4 ? (int)blockIdx.y : 0;
    const int pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
    // k4 / s2 / p1: input slice iz = 2a + pz meets kz = 1 - pz + 2 jz at output slice a + pz - jz (rows and columns alike)
    const int qd = K == 4 ? (a.ID - pz + 1) >> 1 : a.ID, qh = K == 4 ? (a.IH - py + 1) >> 1 : a.IH,
              qw = K == 4 ? (a.IW - px + 1) >> 1 : a.IW;
    const int total = a.N * qd * qh * qw;                  // host guarantees < 2^31 - the grid's stride
    const int nck = (a.Cout + E3_DCH - 1) / E3_DCH;
    bool staged = false;
    for (int p0 = blockIdx.x * 256; p0 < total; p0 += gridDim.x * 256) {
        const int p = p0 + threadIdx.x;
        const bool live = p < total;
        const int b = p % qw;
        int r = p / qw;
        const int aa = r % qh; r /= qh;
        const int ad = r % qd;
        const int n = r / qd;
        float acc[CP];
#pragma unroll
        for (int ci = 0; ci < CP; ++ci) acc[ci] = 0.f;
        for (int ck = 0; ck < nck; ++ck) {
            const int co0 = ck * E3_DCH;
            const int cn = a.Cout - co0 < E3_DCH ? a.Cout - co0 : E3_DCH;
            if (nck > 1 || !staged) {                      // block-uniform: one chunk is staged once, two are restaged per voxel batch
                __syncthreads();
                for (int i = threadIdx.x; i < NTAP * cn * CP; i += 256) {
                    const int ci = i % CP, q = i / CP, co = q % cn, t = q / cn;
                    const int kz = K == 4 ? 1 - pz + 2 * (t >> 2) : 0, ky = K == 4 ? 1 - py + 2 * ((t >> 1) & 1) : 0,
                              kx = K == 4 ? 1 - px + 2 * (t & 1) : 0;
                    wl[(t * E3_DCH + co) * CP + ci] =
                        ci < a.Cin ? a.w[((int64_t)(co0 + co) * a.Cin + ci) * KKK + (kz * K + ky) * K + kx] : 0.f;
                }
                __syncthreads();
                staged = true;
            }
            if (!live) continue;
#pragma unroll
            for (int t = 0; t < NTAP; ++t) {
                const int oz = K == 4 ? ad + pz - (t >> 2) : ad, oy = K == 4 ? aa + py - ((t >> 1) & 1) : aa,
                          ox = K == 4 ? b + px - (t & 1) : b;
                if ((unsigned)oz >= (unsigned)a.OD || (unsigned)oy >= (unsigned)a.OH || (unsigned)ox >= (unsigned)a.OW) continue;
                const unsigned short* dp = a.dy + ((((int64_t)n * a.OD + oz) * a.OH + oy) * a.OW + ox) * a.Cout + co0;
                const float* wt = wl + t * E3_DCH * CP;
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
            const int iz = K == 4 ? 2 * ad + pz : ad, iy = K == 4 ? 2 * aa + py : aa, ix = K == 4 ? 2 * b + px : b;
#pragma unroll
            for (int ci = 0; ci < CP; ++ci)
                if (ci < a.Cin) a.dx[((((int64_t)n * a.Cin + ci) * a.ID + iz) * a.IH + iy) * a.IW + ix] = acc[ci] * a.gscale;
        }
    }
}

// k: 4 or 1 when the geometry is one of the two covered, else 0
int e3_geom(int k, int stride, int pad) {
    if (k == 4 && stride == 2 && pad == 1) return 4;
    if (k == 1 && stride == 1 && pad == 0) return 1;
    return 0;
}

// the image side's dims; a k1 conv is pointwise: its depth is folded into the rows
struct E3Dims { int ID, IH, IW, OD, OH, OW; };

int e3_check(const char* who, const void* p16, const void* f0, const void* f1, int N, int Cin, int Cout, int k, int stride, int pad,
             int dtype, E3Dims& d) {
    GS_CHECK_ARG(p16 && f0 && f1, "%s: null pointer", who);
    GS_CHECK_ARG(((uintptr_t)p16 & 15) == 0 && (((uintptr_t)f0 | (uintptr_t)f1) & 3) == 0,
                 "%s: the 16-bit tensor must be 16-byte aligned, the fp32 tensors 4-byte aligned", who);
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "%s: bad dtype", who);
    GS_CHECK_ARG(N > 0 && d.ID > 0 && d.IH > 0 && d.IW > 0 && d.OD > 0 && d.OH > 0 && d.OW > 0, "%s: bad dims", who);
    if (Cin < 1 || Cin > 16 || Cout < 8 || Cout > 128 || Cout % 8 != 0 || !e3_geom(k, stride, pad)) return GS_EUNSUPPORTED;
    const int e = 2 * pad - k;
    GS_CHECK_ARG(d.ID + e >= 0 && d.IH + e >= 0 && d.IW + e >= 0 && d.OD == (d.ID + e) / stride + 1 && d.OH == (d.IH + e) / stride + 1 &&
                     d.OW == (d.IW + e) / stride + 1,
                 "%s: output size mismatch", who);
    GS_CHECK_ARG((int64_t)N * d.OD * cdiv(d.OH, E3_WPH) * cdiv(d.OW, E3_PW) < 2147483647LL &&
                     (int64_t)N * d.ID * d.IH * d.IW < 2147483647LL - 512 * 256,
                 "%s: too many voxels", who);
    if (k == 1) {
        d.IH *= d.ID; d.OH *= d.OD;
        d.ID = d.OD = 1;
    }
    return GS_OK;
}

int e3_wgrad_blocks(int N, const E3Dims& d) {
    const int64_t np = (int64_t)N * d.OD * cdiv(d.OH, E3_WPH) * cdiv(d.OW, E3_PW);
    return (int)(np < E3_WGRID ? np : E3_WGRID);
}

// ------------------------------------------------------------------------------------------------ one-channel head
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

#define E3_DISPATCH(KERNEL, grid, ...)                                                        \
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

extern "C" int gs_conv3d_img_fwd(const float* x, const float* w, const float* bias, void* y, int N, int Cin, int ID, int IH, int IW,
                                 int Cout, int OD, int OH, int OW, int k, int stride, int pad, int act, int dtype, void* stream) {
    E3Dims d{ID, IH, IW, OD, OH, OW};
    int rc = e3_check("gs_conv3d_img_fwd", y, x, w, N, Cin, Cout, k, stride, pad, dtype, d);
    if (rc) return rc;
    GS_CHECK_ARG(((uintptr_t)bias & 3) == 0, "gs_conv3d_img_fwd: misaligned bias");
    if (act != GS_ACT_NONE && act != GS_ACT_LEAKY02) return GS_EUNSUPPORTED;
    const int kg = e3_geom(k, stride, pad);
    const int tiles_x = cdiv(d.OW, E3_PW), tiles_y = cdiv(d.OH, E3_FPH);
    E3FArgs a{x, w, bias, (unsigned short*)y, N, Cin, d.ID, d.IH, d.IW, Cout, d.OD, d.OH, d.OW, tiles_x, tiles_y, act};
    hipStream_t s = (hipStream_t)stream;
    const int nb = N * d.OD * tiles_y * tiles_x;
    E3_DISPATCH(e3_fwd_kernel, nb, a);
    GS_CHECK_LAUNCH("gs_conv3d_img_fwd");
    return GS_OK;
}

extern "C" int64_t gs_conv3d_img_wgrad_ws_floats(int N, int OD, int OH, int OW, int Cin, int Cout, int k) {
    if (N <= 0 || OD <= 0 || OH <= 0 || OW <= 0 || Cin <= 0 || Cout <= 0 || (k != 4 && k != 1)) return 0;
    if ((int64_t)N * OD * OH >= 2147483647LL) return 0;
    E3Dims d{1, 1, 1, OD, OH, OW};
    if (k == 1) { d.OH *= OD; d.OD = 1; }
    return (int64_t)e3_wgrad_blocks(N, d) * (k == 4 ? E3WGeo<4>::PP : E3WGeo<1>::PP) * Cout * Cin * k * k * k;
}

extern "C" int gs_conv3d_img_wgrad(const float* x, const void* dy, float* dw, float* ws, int N, int Cin, int ID, int IH, int IW, int Cout,
                                   int OD, int OH, int OW, int k, int stride, int pad, float gscale, int dtype, void* stream) {
    E3Dims d{ID, IH, IW, OD, OH, OW};
    int rc = e3_check("gs_conv3d_img_wgrad", dy, x, dw, N, Cin, Cout, k, stride, pad, dtype, d);
    if (rc) return rc;
    GS_CHECK_ARG(ws && ((uintptr_t)ws & 3) == 0, "gs_conv3d_img_wgrad: null or misaligned workspace");
    const int kg = e3_geom(k, stride, pad);
    const int tiles_x = cdiv(d.OW, E3_PW), tiles_y = cdiv(d.OH, E3_WPH);
    E3WArgs a{x, (const unsigned short*)dy, ws, N, Cin, d.ID, d.IH, d.IW, Cout, d.OD, d.OH, d.OW, tiles_x, tiles_y,
              N * d.OD * tiles_y * tiles_x};
    hipStream_t s = (hipStream_t)stream;
    const int gx = e3_wgrad_blocks(N, d);
    const dim3 grid(gx, kg == 4 ? cdiv(Cin, E3WGeo<4>::CW) : 1);
    E3_DISPATCH(e3_wgrad_kernel, grid, a);
    const int n = Cout * Cin * k * k * k;
    e3_slab_sum_kernel<<<cdiv(n, 32), 256, 0, s>>>(ws, gx * (kg == 4 ? E3WGeo<4>::PP : E3WGeo<1>::PP), n, gscale, dw);
    GS_CHECK_LAUNCH("gs_conv3d_img_wgrad");
    return GS_OK;
}

extern "C" int gs_conv3d_img_dgrad(const void* dy, const float* w, float* dx, int N, int Cin, int ID, int IH, int IW, int Cout, int OD,
                                   int OH, int OW, int k, int stride, int pad, float gscale, int dtype, void* stream) {
    E3Dims d{ID, IH, IW, OD, OH, OW};
    int rc = e3_check("gs_conv3d_img_dgrad", dy, w, dx, N, Cin, Cout, k, stride, pad, dtype, d);
    if (rc) return rc;
    const int kg = e3_geom(k, stride, pad);
    E3DArgs a{(const unsigned short*)dy, w, dx, N, Cin, d.ID, d.IH, d.IW, Cout, d.OD, d.OH, d.OW, gscale};
    hipStream_t s = (hipStream_t)stream;
    const int64_t per = kg == 4 ? (int64_t)N * ((d.ID + 1) / 2) * ((d.IH + 1) / 2) * ((d.IW + 1) / 2) : (int64_t)N * d.ID * d.IH * d.IW;
    const int64_t nb64 = cdiv64(per, 256);
    const dim3 grid((int)(nb64 < 512 ? nb64 : 512), kg == 4 ? 8 : 1);
#define E3_DGRAD_CP(DT, CP)                                                    \
    do {                                                                       \
        if (kg == 4) e3_dgrad_kernel<DT, CP, 4><<<grid, 256, 0, s>>>(a);       \
        else e3_dgrad_kernel<DT, CP, 1><<<grid, 256, 0, s>>>(a);               \
    } while (0)
#define E3_DGRAD(DT)                               \
    do {                                           \
        if (Cin <= 2) E3_DGRAD_CP(DT, 2);          \
        else if (Cin <= 4) E3_DGRAD_CP(DT, 4);     \
        else if (Cin <= 8) E3_DGRAD_CP(DT, 8);     \
        else E3_DGRAD_CP(DT, 16);                  \
    } while (0)
    if (dtype == GS_F16) E3_DGRAD(GS_F16);
    else E3_DGRAD(GS_BF16);
#undef E3_DGRAD
#undef E3_DGRAD_CP
    GS_CHECK_LAUNCH("gs_conv3d_img_dgrad");
    return GS_OK;
}

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
