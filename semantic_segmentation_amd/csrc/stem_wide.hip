// The first conv of the pair forward for ANY input channel count (unet/unet_model.py:8-24 with n_channels > 4; the depth-unfolded
// first conv of GenSeg-3D/UNet3D/unet3d.py:89-126 with in_channels > 1): 3x3, stride 1, pad 1, fp32 NCHW image and fp32 weights
// in the reference layout -> dense conv-output pair [N,H,W,Cout] + BatchNorm partial rows.
//
// The image is NOT rounded to 16 bits: that costs 3e-4 (fp16) to 2.5e-3 (bf16) of the conv output, 45 to 100 times pair_tol
// (tests/test_wide_ends_reference_cpu.py).  The products are fp32 x fp32 accumulated in fp32, on the fp32-input MFMA
// v_mfma_f32_32x32x2_f32, which is bit-identical to a k-ordered fmaf chain and otherwise idle in this step.
//
// Implicit GEMM, one block per 8 x 32 pixel patch:
//   * per chunk of 8 input channels the block stages the patch's fp32 halo [ci][10][34] in LDS -- zeros come from the bounds test
//     here, once, not per tap -- and the matching weight slab [k = (ci, ky, kx)][Cout] (row stride Cout + 1: the staging writes walk
//     k, the MFMA reads walk the channel, both conflict-free).  K is padded to an even count with zero weights over a zero plane.
//   * the MFMA's A operand is the WEIGHT (rows = 32 output channels), its B operand the image (columns = the 32 pixels of a patch
//     row): the accumulator then has the pixel on the lane and channels in the registers, so a lane splits and stores complete
//     16-byte channel groups without a transpose.  A-row r of a tile holds channel 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3), which
//     makes register g of lane half h channel 16 h + g.
//   * wave w owns patch rows 2w, 2w + 1 and every 32-channel tile: 2 * Cout / 32 accumulators, each weight fragment used twice.
//   * statistics: the lane's two rows are added, the block's 128 lanes of a channel transposed through LDS and added in a fixed
//     order.  No atomics: two runs give the same bits.
#include "common.hpp"

namespace {

constexpr int WC_PH = 8, WC_PW = 32;                                  // pixel patch of a block
constexpr int WC_CC = 8;                                              // input channels per chunk
constexpr int WC_HS = WC_PW + 2, WC_PLANE = (WC_PH + 2) * WC_HS;      // halo row stride / plane
constexpr int WC_KC = WC_CC * 9;                                      // K of a full chunk
constexpr int WC_RS = 129;                                            // row stride of the statistics transpose

struct WCArgs {
    const float* x; const float* w; unsigned short* y_hi; unsigned short* y_lo; float* bnp;
    int N, Cin, H, W, Cout, tiles_x, tiles_y;
};

template <int DT, int NT>
__global__ __launch_bounds__(256) void widecin_split_kernel(const WCArgs a) {
    constexpr int WS = NT * 32 + 1;
    __shared__ float lds[WC_CC * WC_PLANE + WC_KC * WS];   // halo | weight slab [k][A row]; then the statistics transpose
    __shared__ int koff[WC_KC];
    float* const halo = lds;
    float* const wl = lds + WC_CC * WC_PLANE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    int t = blockIdx.x;
    const int tx = t % a.tiles_x; t /= a.tiles_x;
    const int ty = t % a.tiles_y;
    const int n = t / a.tiles_y;
    const int x0 = tx * WC_PW, y0 = ty * WC_PH;
    if (threadIdx.x < WC_KC) {
        const int k = threadIdx.x, ci = k / 9, tt = k - ci * 9, ky = tt / 3;
        koff[k] = ci * WC_PLANE + ky * WC_HS + (tt - 3 * ky);
    }
    f32x16 acc[2][NT];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[r][nt][g] = 0.f;

    for (int c0 = 0; c0 < a.Cin; c0 += WC_CC) {
        const int cc = a.Cin - c0 < WC_CC ? a.Cin - c0 : WC_CC;
        const int kc = cc * 9, kcp = (kc + 1) & ~1;
        const int planes = cc + (cc & 1);                  // odd K: one zero plane under the zero weight row (cc odd => cc < WC_CC)
        __syncthreads();                                   // the previous chunk has been read
        for (int i = threadIdx.x; i < planes * WC_PLANE; i += 256) {
            const int ci = i / WC_PLANE, r = i - ci * WC_PLANE;
            const int hy = r / WC_HS, hx = r - hy * WC_HS;
            const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
            float v = 0.f;
            if (ci < cc && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                v = a.x[(((int64_t)n * a.Cin + c0 + ci) * a.H + iy) * a.W + ix];
            halo[i] = v;
        }
        for (int i = threadIdx.x; i < NT * 32 * kcp; i += 256) {
            const int co = i / kcp, k = i - co * kcp;
            const float v = k < kc ? a.w[((int64_t)co * a.Cin + c0) * 9 + k] : 0.f;
            const int c = co & 31;
            wl[k * WS + (co & ~31) + ((c >> 2) & 3) * 8 + (c >> 4) * 4 + (c & 3)] = v;
        }
        __syncthreads();
        const float* hb = halo + 2 * wave * WC_HS + li;
        for (int s = 0; s < kcp; s += 2) {
            const int k = s + lh;
            const float* hp = hb + koff[k];
            const float b0 = hp[0], b1 = hp[WC_HS];
            const float* wp = wl + k * WS + li;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float aw = wp[nt * 32];
                acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, b0, acc[0][nt], 0, 0, 0);
                acc[1][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, b1, acc[1][nt], 0, 0, 0);
            }
        }
    }

    // the lane holds pixel (y0 + 2 wave + r, x0 + li), channels 32 nt + 16 lh + (0..15): two 16-byte groups per plane
    const int px = x0 + li;
    bool live[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int py = y0 + 2 * wave + r;
        live[r] = px < a.W && py < a.H;
        if (live[r]) {
            const int64_t base = (((int64_t)n * a.H + py) * a.W + px) * a.Cout + 16 * lh;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int g8 = 0; g8 < 2; ++g8) {
                    float v8[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v8[i] = acc[r][nt][g8 * 8 + i];
                    uint4 hi, lo;
                    split8<DT>(v8, hi, lo);
                    st16(a.y_hi + base + nt * 32 + g8 * 8, hi);
                    st16(a.y_lo + base + nt * 32 + g8 * 8, lo);
                }
        }
    }
    if (a.bnp) {
        // per 32-channel tile and slot: the 128 pixels-in-lanes of a channel side by side in LDS (row stride 129: conflict-free
        // writes, 2-way reads), thread (q, c) adds 16 of them in order, then one thread per (slot, channel) adds the 8 parts in order
        float* const red = lds;                            // [32 channels][WC_RS]
        float* const part = lds + 32 * WC_RS;              // [NT][2][8][32]
        static_assert(32 * WC_RS + NT * 2 * 256 <= WC_CC * WC_PLANE + WC_KC * WS, "statistics staging exceeds the operand LDS");
        const int c = threadIdx.x & 31, q = threadIdx.x >> 5;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int slot = 0; slot < 2; ++slot) {
                __syncthreads();                           // the K loop / the previous transpose has been read
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const float v0 = live[0] ? acc[0][nt][g] : 0.f, v1 = live[1] ? acc[1][nt][g] : 0.f;
                    red[(16 * lh + g) * WC_RS + wave * 32 + li] = slot == 0 ? v0 + v1 : v0 * v0 + v1 * v1;
                }
                __syncthreads();
                float t = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) t += red[c * WC_RS + q * 16 + i];
                part[((nt * 2 + slot) * 8 + q) * 32 + c] = t;
            }
        __syncthreads();
        if ((int)threadIdx.x < 2 * a.Cout) {
            const int slot = (int)threadIdx.x / a.Cout, ch = (int)threadIdx.x - slot * a.Cout;
            const float* pp = part + (((ch >> 5) * 2 + slot) * 8) * 32 + (ch & 31);
            float t = 0.f;
#pragma unroll
            for (int qq = 0; qq < 8; ++qq) t += pp[qq * 32];
            a.bnp[(int64_t)blockIdx.x * 2 * a.Cout + threadIdx.x] = t;
        }
    }
}

}  // namespace

extern "C" int gs_conv_widecin_mtiles(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t t = (int64_t)N * cdiv(H, WC_PH) * cdiv(W, WC_PW);
    return t < 2147483647LL ? (int)t : 0;
}

extern "C" int gs_conv_widecin_fwd_split(const float* x, const float* w, void* y_hi, void* y_lo, float* bn_partials, int N, int Cin,
                                         int H, int W, int Cout, int dtype, void* stream) {
    GS_CHECK_ARG(x && w && y_hi && y_lo && N > 0 && H > 0 && W > 0, "gs_conv_widecin_fwd_split: bad arguments");
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "gs_conv_widecin_fwd_split: bad dtype");
    if (Cin < 1 || Cin > 64 || Cout < 32 || Cout > 128 || Cout % 32 != 0) return GS_EUNSUPPORTED;
    GS_CHECK_ARG((((uintptr_t)y_hi | (uintptr_t)y_lo) & 15) == 0, "gs_conv_widecin_fwd_split: y_hi / y_lo must be 16-byte aligned");
    const int nb = gs_conv_widecin_mtiles(N, H, W);
    GS_CHECK_ARG(nb > 0, "gs_conv_widecin_fwd_split: too many pixels");
    WCArgs a{x, w, (unsigned short*)y_hi, (unsigned short*)y_lo, bn_partials, N, Cin, H, W, Cout, cdiv(W, WC_PW), cdiv(H, WC_PH)};
    hipStream_t s = (hipStream_t)stream;
#define GS_WIDECIN(NT)                                                                   \
    do {                                                                                 \
        if (dtype == GS_F16) widecin_split_kernel<GS_F16, NT><<<nb, 256, 0, s>>>(a);     \
        else widecin_split_kernel<GS_BF16, NT><<<nb, 256, 0, s>>>(a);                    \
    } while (0)
    switch (Cout / 32) {
        case 1: GS_WIDECIN(1); break;
        case 2: GS_WIDECIN(2); break;
        case 3: GS_WIDECIN(3); break;
        default: GS_WIDECIN(4); break;
    }
#undef GS_WIDECIN
    GS_CHECK_LAUNCH("gs_conv_widecin_fwd_split");
    return GS_OK;
}
