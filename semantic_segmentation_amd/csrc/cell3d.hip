// The two operators of the 3-D Pix2Pix generator that the generic engine cannot take as they are (GenSeg-3D/models/networks.py:50-81
// LinearAdditiveUpsample, :570-601 MixedOp_conv / Cell_conv over architecture_pix2pix/operations.py:41-66 conv_421 / 622 / 823).
//
// Mixed cell.  sum_j sm_j Conv3d_j(x), (k, s, p) = (4,2,1), (6,2,2), (8,2,3), is ONE 8x8x8 / stride 2 / pad 3 conv (k4 embedded at
// offset 2, k6 at offset 1): 512 taps, eight times GS_MAX_TAPS.  Per axis it reads x[2o + k - 3]; with k - 2 = 2 dt + p, p in {0,1},
// dt in {-1,0,1,2}, that is x[2(o + dt) + p - 1].  On the parity-gathered tensor
//     x'[a, (pz,py,px,c)] = x[2a+pz-1, 2i+py-1, 2j+px-1, c]            (zero outside the volume, ceil((D+1)/2) entries per axis)
// the cell is a STRIDE-1 conv of 4x4x4 = 64 taps over 8 Cin channels, which gs_conv_igemm / gs_conv_wgrad_slabs run as they are; the
// data gradient goes to x directly through the eight 64-tap sub-voxel classes of the stride-2 conv.  Here: the gather, the merge of
// the three weights into the packs of both launches (only the taps that can meet data, see the box arguments), and the split of the
// merged weight gradient back into dW4 / dW6 / dW8 and the three architecture dot products.
//
// Additive upsample.  Trilinear x2 (align_corners=False: output 2i = 0.25 x[i-1] + 0.75 x[i], 2i+1 = 0.75 x[i] + 0.25 x[i+1], indices
// clamped) of the sum of each 4 consecutive channels, and its exact adjoint in gather form.  Memory bound: 16-byte accesses along C.
#include "common.hpp"

namespace {

int grid_for(int64_t total, int cap = 16384) {
    int64_t b = cdiv64(total, 256);
    return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// ------------------------------------------------------------------------------------------------ gather
struct GatherArgs {
    const unsigned short* x16; const float* x32; unsigned short* out;
    int N, D, H, W, Cin, xs, xc, GD, GH, GW;
};

__global__ __launch_bounds__(256) void gather16_kernel(const GatherArgs a) {
    const int nch = a.Cin >> 3;
    const int64_t total = (int64_t)a.N * a.GD * a.GH * a.GW * 8 * nch;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int ch = (int)(idx % nch);
        int64_t p = idx / nch;
        const int q = (int)(p & 7); p >>= 3;
        const int j = (int)(p % a.GW); p /= a.GW;
        const int i = (int)(p % a.GH); p /= a.GH;
        const int d = (int)(p % a.GD);
        const int n = (int)(p / a.GD);                 // the depth slices of sample n only: z is tested against D, not N*D
        const int z = 2 * d + (q >> 2) - 1, y = 2 * i + ((q >> 1) & 1) - 1, x = 2 * j + (q & 1) - 1;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if ((unsigned)z < (unsigned)a.D && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W)
            v = *reinterpret_cast<const uint4*>(a.x16 + ((((int64_t)n * a.D + z) * a.H + y) * a.W + x) * a.xs + a.xc + ch * 8);
        st16(a.out + idx * 8, v);                      // channel q*Cin + 8 ch of voxel (n,d,i,j): exactly element 8 idx
    }
}

// fp32 NCDHW image, Cin 1..4: 8 Cin gathered channels = Cin chunks of 8; channel g = q*Cin + c.  Rounded once to 16 bits.
template <int DT>
__global__ __launch_bounds__(256) void gather32_kernel(const GatherArgs a) {
    const int64_t total = (int64_t)a.N * a.GD * a.GH * a.GW * a.Cin;
    const int64_t plane = (int64_t)a.H * a.W;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int k = (int)(idx % a.Cin);
        int64_t p = idx / a.Cin;
        const int j = (int)(p % a.GW); p /= a.GW;
        const int i = (int)(p % a.GH); p /= a.GH;
        const int d = (int)(p % a.GD);
        const int n = (int)(p / a.GD);
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int g = 8 * k + e, q = g / a.Cin, c = g - q * a.Cin;
            const int z = 2 * d + (q >> 2) - 1, y = 2 * i + ((q >> 1) & 1) - 1, x = 2 * j + (q & 1) - 1;
            f[e] = 0.f;
            if ((unsigned)z < (unsigned)a.D && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W)
                f[e] = a.x32[(((int64_t)n * a.Cin + c) * a.D + z) * plane + (int64_t)y * a.W + x];
        }
        st16(a.out + idx * 8, pack8<DT>(f));
    }
}

// ------------------------------------------------------------------------------------------------ merge
struct MergeArgs {
    const float *w4, *w6, *w8, *sm;
    unsigned short *pf, *pd;
    int Cin, Cout, cinp;
    int dt0[3], nd[3], k0[3], nk[3];
};

// sm0 W4 (embedded at offset 2) + sm1 W6 (offset 1) + sm2 W8 at tap (kz,ky,kx): summed in this order in fp32
__device__ __forceinline__ float merged_at(const MergeArgs& a, int co, int ci, int kz, int ky, int kx, float s0, float s1, float s2) {
    const int64_t oc = (int64_t)co * a.Cin + ci;
    const int z4 = kz - 2, y4 = ky - 2, x4 = kx - 2, z6 = kz - 1, y6 = ky - 1, x6 = kx - 1;
    float t4 = 0.f, t6 = 0.f;
    if ((unsigned)z4 < 4u && (unsigned)y4 < 4u && (unsigned)x4 < 4u) t4 = a.w4[oc * 64 + z4 * 16 + y4 * 4 + x4];
    if ((unsigned)z6 < 6u && (unsigned)y6 < 6u && (unsigned)x6 < 6u) t6 = a.w6[oc * 216 + z6 * 36 + y6 * 6 + x6];
    const float t8 = a.w8[oc * 512 + kz * 64 + ky * 8 + kx];
    return (s0 * t4 + s1 * t6) + s2 * t8;
}

// Both packs through one tile kernel.  A block owns one "major" channel (forward: co, data gradient: ci) and up to 32 "minor" channels
// (forward: ci, data gradient: co): for each of them the taps of the box are a few contiguous runs of the fp32 weights, so the reads
// are coalesced; the merged, rounded values go through LDS as [tap][minor] and leave as 64-byte runs along the pack's innermost axis.
//   forward pack [nd taps][Cout][8 Cin], gathered channel order (pz,py,px,c); tap (dtz,dty,dtx), parity p: k = 2 dt + p + 2, so the
//     box of k is 2 dt0 + 2 .. 2 (dt0 + nd) + 1 and a local tap index l gives dt - dt0 = l >> 1, p = l & 1;
//   data-gradient pack [nk taps][cinp][Cout] over k0 .. k0 + nk; rows ci >= Cin (the image side padded to 8) are zero.
constexpr int MG_CH = 32;

template <int DT, bool DGRAD>
__global__ __launch_bounds__(256) void merge_tile_kernel(const MergeArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned short tile[512 * MG_CH];
    const int nminor = DGRAD ? a.Cout : a.Cin;
    const int nmb = (nminor + MG_CH - 1) / MG_CH;
    const int major = blockIdx.x / nmb, m0 = (blockIdx.x % nmb) * MG_CH;
    const int nm = min(MG_CH, nminor - m0);
    const int b0 = DGRAD ? a.k0[0] : 2 * a.dt0[0] + 2, b1 = DGRAD ? a.k0[1] : 2 * a.dt0[1] + 2, b2 = DGRAD ? a.k0[2] : 2 * a.dt0[2] + 2;
    const int n0 = DGRAD ? a.nk[0] : 2 * a.nd[0], n1 = DGRAD ? a.nk[1] : 2 * a.nd[1], n2 = DGRAD ? a.nk[2] : 2 * a.nd[2];
    const int nk = n0 * n1 * n2;                      // <= 512
    const float s0 = a.sm[0], s1 = a.sm[1], s2 = a.sm[2];
    const bool zero_row = DGRAD && major >= a.Cin;
    for (int e = threadIdx.x; e < nm * nk; e += 256) {
        const int m = e / nk, lk = e - m * nk;
        const int kx = b2 + lk % n2, ky = b1 + (lk / n2) % n1, kz = b0 + lk / (n1 * n2);
        const int co = DGRAD ? m0 + m : major, ci = DGRAD ? major : m0 + m;
        tile[lk * MG_CH + m] = Elem<DT>::from_f(zero_row ? 0.f : merged_at(a, co, ci, kz, ky, kx, s0, s1, s2));
    }
    __syncthreads();
    if (DGRAD) {                                      // the local tap index IS the pack's; Cout % 8 == 0, so nm % 8 == 0
        const int nv = nm >> 3;
        for (int e = threadIdx.x; e < nk * nv; e += 256) {
            const int lk = e / nv, v = e - lk * nv;
            st16(a.pd + ((int64_t)lk * a.cinp + major) * a.Cout + m0 + v * 8, *reinterpret_cast<const uint4*>(&tile[lk * MG_CH + v * 8]));
        }
        return;
    }
    const int c8 = 8 * a.Cin;
    const bool vec = (a.Cin & 7) == 0;
    const int per = vec ? nm >> 3 : nm;               // stores per tap: 16-byte chunks, or single elements for the image side
    for (int e = threadIdx.x; e < nk * per; e += 256) {
        const int lk = e / per, v = e - lk * per;
        const int lx = lk % n2, ly = (lk / n2) % n1, lz = lk / (n1 * n2);
        const int t = ((lz >> 1) * a.nd[1] + (ly >> 1)) * a.nd[2] + (lx >> 1);
        const int q = ((lz & 1) << 2) | ((ly & 1) << 1) | (lx & 1);
        unsigned short* dst = a.pf + ((int64_t)t * a.Cout + major) * c8 + q * a.Cin + m0;
        if (vec) st16(dst + v * 8, *reinterpret_cast<const uint4*>(&tile[lk * MG_CH + v * 8]));
        else dst[v] = tile[lk * MG_CH + v];
    }
}

// ------------------------------------------------------------------------------------------------ split
struct SplitArgs {
    const float *dwm, *w4, *w6, *w8, *sm;
    float *dw4, *dw6, *dw8, *dots, *ws;
    float gscale;
    int Cin, Cout, nblocks;
    int dt0[3], nd[3];
};

// A block owns one co and up to 16 ci: it reads its share of dwm (64-byte runs along the gathered channels) into LDS as [k of 512][ci]
// -- taps outside the box never meet data: their gradient is zero -- and writes the three gradients along their own innermost axis;
// per-block partial dot products go to ws[block][3], summed in block order by split_dots_kernel
constexpr int SP_CH = 16;

__global__ __launch_bounds__(256) void split_wgrad_kernel(const SplitArgs a) {
    __shared__ float tile[512 * SP_CH];
    __shared__ float red[4];
    const int nmb = (a.Cin + SP_CH - 1) / SP_CH;
    const int co = blockIdx.x / nmb, m0 = (blockIdx.x % nmb) * SP_CH;
    const int nm = min(SP_CH, a.Cin - m0);
    const float s0 = a.sm[0], s1 = a.sm[1], s2 = a.sm[2];
    const int c8 = 8 * a.Cin;
    const int nt = a.nd[0] * a.nd[1] * a.nd[2];
    for (int e = threadIdx.x; e < 512 * SP_CH; e += 256) tile[e] = 0.f;
    __syncthreads();
    for (int e = threadIdx.x; e < nt * 8 * nm; e += 256) {
        const int m = e % nm, r = e / nm;
        const int q = r & 7, t = r >> 3;
        const int tx = t % a.nd[2], ty = (t / a.nd[2]) % a.nd[1], tz = t / (a.nd[1] * a.nd[2]);
        const int kz = 2 * (a.dt0[0] + tz) + (q >> 2) + 2, ky = 2 * (a.dt0[1] + ty) + ((q >> 1) & 1) + 2, kx = 2 * (a.dt0[2] + tx) + (q & 1) + 2;
        tile[(kz * 64 + ky * 8 + kx) * SP_CH + m] = a.dwm[((int64_t)t * a.Cout + co) * c8 + q * a.Cin + m0 + m];
    }
    __syncthreads();
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    for (int e = threadIdx.x; e < nm * 512; e += 256) {
        const int m = e >> 9, k = e & 511;
        const int kz = k >> 6, ky = (k >> 3) & 7, kx = k & 7;
        const float v = tile[k * SP_CH + m];
        const int64_t oc = (int64_t)co * a.Cin + m0 + m;
        const int64_t idx = oc * 512 + k;
        a.dw8[idx] = a.gscale * s2 * v;
        p2 += v * a.w8[idx];
        const int z6 = kz - 1, y6 = ky - 1, x6 = kx - 1;
        if ((unsigned)z6 < 6u && (unsigned)y6 < 6u && (unsigned)x6 < 6u) {
            const int64_t o6 = oc * 216 + z6 * 36 + y6 * 6 + x6;
            a.dw6[o6] = a.gscale * s1 * v;
            p1 += v * a.w6[o6];
        }
        const int z4 = kz - 2, y4 = ky - 2, x4 = kx - 2;
        if ((unsigned)z4 < 4u && (unsigned)y4 < 4u && (unsigned)x4 < 4u) {
            const int64_t o4 = oc * 64 + z4 * 16 + y4 * 4 + x4;
            a.dw4[o4] = a.gscale * s0 * v;
            p0 += v * a.w4[o4];
        }
    }
    p0 = block_sum_256(p0, red);
    p1 = block_sum_256(p1, red);
    p2 = block_sum_256(p2, red);
    if (threadIdx.x == 0) {
        a.ws[blockIdx.x * 3 + 0] = p0; a.ws[blockIdx.x * 3 + 1] = p1; a.ws[blockIdx.x * 3 + 2] = p2;
    }
}

__global__ __launch_bounds__(256) void split_dots_kernel(const SplitArgs a) {
    __shared__ float red[4];
    for (int j = 0; j < 3; ++j) {
        float p = 0.f;
        for (int b = threadIdx.x; b < a.nblocks; b += 256) p += a.ws[b * 3 + j];
        p = block_sum_256(p, red);
        if (threadIdx.x == 0) a.dots[j] = a.gscale * p;
    }
}

// ------------------------------------------------------------------------------------------------ additive upsample
struct UpAddArgs {
    const unsigned short* x; unsigned short* y;       // fwd: x -> y;  bwd: x = dY (read), y = dX (written)
    int N, D, H, W, C, lo_s, lo_c, hi_s, hi_c;         // low-resolution tensor [N*D,H,W,C]; high-resolution [N*2D,2H,2W,C/4]
};

// sources and weights of output o on an axis of n entries
__device__ __forceinline__ void up_axis(int o, int n, int& i0, int& i1, float& w0, float& w1) {
    const int i = o >> 1;
    if (o & 1) { i0 = i; i1 = min(i + 1, n - 1); w0 = 0.75f; w1 = 0.25f; }
    else { i0 = max(i - 1, 0); i1 = i; w0 = 0.25f; w1 = 0.75f; }
}

template <int DT>
__global__ __launch_bounds__(256) void upadd_fwd_kernel(const UpAddArgs a) {
    const int nch = a.C >> 5;                          // 32 input channels -> 8 output channels per thread
    const int OD = 2 * a.D, OH = 2 * a.H, OW = 2 * a.W;
    const int64_t total = (int64_t)a.N * OD * OH * OW * nch;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int ch = (int)(idx % nch);
        int64_t p = idx / nch;
        const int ox = (int)(p % OW); p /= OW;
        const int oy = (int)(p % OH); p /= OH;
        const int oz = (int)(p % OD);
        const int n = (int)(p / OD);
        int iz[2], iy[2], ix[2];
        float wz[2], wy[2], wx[2];
        up_axis(oz, a.D, iz[0], iz[1], wz[0], wz[1]);
        up_axis(oy, a.H, iy[0], iy[1], wy[0], wy[1]);
        up_axis(ox, a.W, ix[0], ix[1], wx[0], wx[1]);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int z = iz[c >> 2], y = iy[(c >> 1) & 1], x = ix[c & 1];
            const float w = wz[c >> 2] * wy[(c >> 1) & 1] * wx[c & 1];
            const unsigned short* src = a.x + ((((int64_t)n * a.D + z) * a.H + y) * a.W + x) * a.lo_s + a.lo_c + ch * 32;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float f[8];
                unpack8<DT>(*reinterpret_cast<const uint4*>(src + 8 * k), f);
                acc[2 * k] += w * ((f[0] + f[1]) + (f[2] + f[3]));
                acc[2 * k + 1] += w * ((f[4] + f[5]) + (f[6] + f[7]));
            }
        }
        const int64_t pix = (((int64_t)n * OD + oz) * OH + oy) * OW + ox;
        st16(a.y + pix * a.hi_s + a.hi_c + ch * 8, pack8<DT>(acc));
    }
}

// outputs that read input i on an axis of n entries: 2i-1 .. 2i+2 with weights 0.25, 0.75, 0.75, 0.25; the clamp folds the missing
// neighbour's quarter onto the edge entry (output 0 equals x[0])
__device__ __forceinline__ void up_axis_adj(int i, int n, float (&w)[4]) {
    w[0] = i >= 1 ? 0.25f : 0.f;
    w[1] = i == 0 ? 1.f : 0.75f;
    w[2] = i == n - 1 ? 1.f : 0.75f;
    w[3] = i < n - 1 ? 0.25f : 0.f;
}

template <int DT>
__global__ __launch_bounds__(256) void upadd_bwd_kernel(const UpAddArgs a) {
    const int nch = a.C >> 5;
    const int OD = 2 * a.D, OH = 2 * a.H, OW = 2 * a.W;
    const int64_t total = (int64_t)a.N * a.D * a.H * a.W * nch;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int ch = (int)(idx % nch);
        int64_t p = idx / nch;
        const int ix = (int)(p % a.W); p /= a.W;
        const int iy = (int)(p % a.H); p /= a.H;
        const int iz = (int)(p % a.D);
        const int n = (int)(p / a.D);
        float wz[4], wy[4], wx[4];
        up_axis_adj(iz, a.D, wz);
        up_axis_adj(iy, a.H, wy);
        up_axis_adj(ix, a.W, wx);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int tz = 0; tz < 4; ++tz) {
            if (wz[tz] == 0.f) continue;
            const int oz = 2 * iz - 1 + tz;
            for (int ty = 0; ty < 4; ++ty) {
                if (wy[ty] == 0.f) continue;
                const int oy = 2 * iy - 1 + ty;
                for (int tx = 0; tx < 4; ++tx) {
                    if (wx[tx] == 0.f) continue;
                    const int ox = 2 * ix - 1 + tx;
                    const int64_t pix = (((int64_t)n * OD + oz) * OH + oy) * OW + ox;
                    float g[8];
                    unpack8<DT>(*reinterpret_cast<const uint4*>(a.x + pix * a.hi_s + a.hi_c + ch * 8), g);
                    const float w = wz[tz] * wy[ty] * wx[tx];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += w * g[e];
                }
            }
        }
        unsigned short* dst = a.y + ((((int64_t)n * a.D + iz) * a.H + iy) * a.W + ix) * a.lo_s + a.lo_c + ch * 32;
#pragma unroll
        for (int k = 0; k < 4; ++k) {                  // the four members of a group get the same value
            const unsigned int lo = Elem<DT>::pack2(acc[2 * k], acc[2 * k]), hi = Elem<DT>::pack2(acc[2 * k + 1], acc[2 * k + 1]);
            st16(dst + 8 * k, make_uint4(lo, lo, hi, hi));
        }
    }
}

int check_cell_channels(const char* who, int Cin, int Cout) {
    if (!((Cin >= 1 && Cin <= 4) || (Cin > 0 && Cin % 8 == 0)) || Cout <= 0 || Cout % 8 != 0) {
        gs_set_error("%s: C_in=%d must be 1..4 or a multiple of 8, C_out=%d a multiple of 8", who, Cin, Cout);
        return GS_EUNSUPPORTED;
    }
    return GS_OK;
}

int check_upadd(const char* who, const void* lo, const void* hi, int N, int D, int H, int W, int C, int lo_s, int lo_c, int hi_s,
                int hi_c, int dtype) {
    GS_CHECK_ARG(lo && hi && lo != hi, "%s: null pointer", who);
    GS_CHECK_ARG(aligned(lo, 16) && aligned(hi, 16), "%s: tensors must be 16-byte aligned", who);
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "%s: bad dtype %d", who, dtype);
    GS_CHECK_ARG(N > 0 && D > 0 && H > 0 && W > 0, "%s: non-positive dims", who);
    if (C <= 0 || C % 32 != 0) {
        gs_set_error("%s: C=%d must be a multiple of 32 (groups of 4 channels, 16-byte chunks of C/4)", who, C);
        return GS_EUNSUPPORTED;
    }
    GS_CHECK_ARG(lo_s >= lo_c + C && lo_s % 8 == 0 && lo_c % 8 == 0 && lo_c >= 0, "%s: bad low-resolution stride/offset (%d,%d)", who, lo_s, lo_c);
    GS_CHECK_ARG(hi_s >= hi_c + C / 4 && hi_s % 8 == 0 && hi_c % 8 == 0 && hi_c >= 0, "%s: bad high-resolution stride/offset (%d,%d)", who, hi_s, hi_c);
    GS_CHECK_ARG((int64_t)N * 8 * D * H * W < 2147483000LL, "%s: too many voxels", who);
    return GS_OK;
}

}  // namespace

extern "C" int gs_cell3d_gather(const void* x16, const float* x32, void* out, int N, int D, int H, int W, int Cin, int in_pix_stride,
                                int in_coff, int dtype, void* stream) {
    GS_CHECK_ARG(out != nullptr && ((x16 != nullptr) != (x32 != nullptr)), "gs_cell3d_gather: exactly one source, and an output");
    GS_CHECK_ARG(aligned(out, 16) && aligned(x16, 16) && aligned(x32, 4), "gs_cell3d_gather: misaligned pointer");
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "gs_cell3d_gather: bad dtype %d", dtype);
    GS_CHECK_ARG(N > 0 && D >= 2 && H >= 2 && W >= 2, "gs_cell3d_gather: every spatial size must be >= 2");
    if (x16 ? !(Cin > 0 && Cin % 8 == 0) : !(Cin >= 1 && Cin <= 4)) {
        gs_set_error("gs_cell3d_gather: C_in=%d: a 16-bit source takes a multiple of 8, an fp32 volume 1..4", Cin);
        return GS_EUNSUPPORTED;
    }
    if (x16)
        GS_CHECK_ARG(in_pix_stride >= in_coff + Cin && in_pix_stride % 8 == 0 && in_coff % 8 == 0 && in_coff >= 0,
                     "gs_cell3d_gather: input stride/offset (%d,%d) must cover C_in=%d and be multiples of 8", in_pix_stride, in_coff, Cin);
    GatherArgs a{};
    a.x16 = (const unsigned short*)x16; a.x32 = x32; a.out = (unsigned short*)out;
    a.N = N; a.D = D; a.H = H; a.W = W; a.Cin = Cin; a.xs = in_pix_stride; a.xc = in_coff;
    a.GD = (D + 2) / 2; a.GH = (H + 2) / 2; a.GW = (W + 2) / 2;
    GS_CHECK_ARG((int64_t)N * D * H * W < 2147483000LL && (int64_t)N * a.GD * a.GH * a.GW < 2147483000LL / 8, "gs_cell3d_gather: too many voxels");
    const int64_t voxels = (int64_t)N * a.GD * a.GH * a.GW;
    if (x16) {
        gather16_kernel<<<grid_for(voxels * Cin), 256, 0, (hipStream_t)stream>>>(a);
    } else if (dtype == GS_F16) {
        gather32_kernel<GS_F16><<<grid_for(voxels * Cin), 256, 0, (hipStream_t)stream>>>(a);
    } else {
        gather32_kernel<GS_BF16><<<grid_for(voxels * Cin), 256, 0, (hipStream_t)stream>>>(a);
    }
    GS_CHECK_LAUNCH("gs_cell3d_gather");
    return GS_OK;
}

extern "C" int gs_cell3d_merge_pack(const float* w4, const float* w6, const float* w8, const float* softmax3, void* pack_fwd,
                                    void* pack_dgrad, int Cin, int Cout, int cin_pad, const int* dt0, const int* nd, const int* k0,
                                    const int* nk, int dtype, void* stream) {
    GS_CHECK_ARG(w4 && w6 && w8 && softmax3 && (pack_fwd || pack_dgrad), "gs_cell3d_merge_pack: null pointer");
    GS_CHECK_ARG(aligned(w4, 4) && aligned(w6, 4) && aligned(w8, 4) && aligned(softmax3, 4) && aligned(pack_fwd, 16) && aligned(pack_dgrad, 16),
                 "gs_cell3d_merge_pack: misaligned pointer");
    GS_CHECK_ARG(dtype == GS_F16 || dtype == GS_BF16, "gs_cell3d_merge_pack: bad dtype %d", dtype);
    int rc = check_cell_channels("gs_cell3d_merge_pack", Cin, Cout);
    if (rc) return rc;
    MergeArgs a{};
    a.w4 = w4; a.w6 = w6; a.w8 = w8; a.sm = softmax3; a.pf = (unsigned short*)pack_fwd; a.pd = (unsigned short*)pack_dgrad;
    a.Cin = Cin; a.Cout = Cout; a.cinp = cin_pad;
    if (pack_fwd) {
        GS_CHECK_ARG(dt0 && nd, "gs_cell3d_merge_pack: the forward pack needs its tap box");
        for (int i = 0; i < 3; ++i) {
            GS_CHECK_ARG(dt0[i] >= -1 && nd[i] >= 1 && dt0[i] + nd[i] <= 3, "gs_cell3d_merge_pack: forward tap box outside -1..2");
            a.dt0[i] = dt0[i]; a.nd[i] = nd[i];
        }
    }
    if (pack_dgrad) {
        GS_CHECK_ARG(k0 && nk, "gs_cell3d_merge_pack: the data-gradient pack needs its tap box");
        GS_CHECK_ARG(cin_pad >= Cin && cin_pad % 8 == 0, "gs_cell3d_merge_pack: cin_pad=%d must be a multiple of 8 that covers C_in=%d", cin_pad, Cin);
        for (int i = 0; i < 3; ++i) {
            GS_CHECK_ARG(k0[i] >= 0 && nk[i] >= 1 && k0[i] + nk[i] <= 8, "gs_cell3d_merge_pack: data-gradient tap box outside 0..7");
            a.k0[i] = k0[i]; a.nk[i] = nk[i];
        }
    }
    GS_CHECK_ARG((int64_t)Cout * cdiv(Cin, MG_CH) < 2147483000LL && (int64_t)cin_pad * cdiv(Cout, MG_CH) < 2147483000LL,
                 "gs_cell3d_merge_pack: too many channels");
    if (pack_fwd) {
        const int g = Cout * cdiv(Cin, MG_CH);
        if (dtype == GS_F16) merge_tile_kernel<GS_F16, false><<<g, 256, 0, (hipStream_t)stream>>>(a);
        else merge_tile_kernel<GS_BF16, false><<<g, 256, 0, (hipStream_t)stream>>>(a);
        GS_CHECK_LAUNCH("gs_cell3d_merge_pack");
    }
    if (pack_dgrad) {
        const int g = cin_pad * cdiv(Cout, MG_CH);
        if (dtype == GS_F16) merge_tile_kernel<GS_F16, true><<<g, 256, 0, (hipStream_t)stream>>>(a);
        else merge_tile_kernel<GS_BF16, true><<<g, 256, 0, (hipStream_t)stream>>>(a);
        GS_CHECK_LAUNCH("gs_cell3d_merge_pack");
    }
    return GS_OK;
}

static int64_t split_blocks(int Cin, int Cout) { return (int64_t)Cout * cdiv(Cin, SP_CH); }

extern "C" int64_t gs_cell3d_split_wgrad_ws_floats(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0) return 0;
    return 3 * split_blocks(Cin, Cout);
}

extern "C" int gs_cell3d_split_wgrad(const float* dwm, const float* w4, const float* w6, const float* w8, const float* softmax3,
                                     float gscale, float* dw4, float* dw6, float* dw8, float* dots3, float* ws, int Cin, int Cout,
                                     const int* dt0, const int* nd, void* stream) {
    GS_CHECK_ARG(dwm && w4 && w6 && w8 && softmax3 && dw4 && dw6 && dw8 && dots3 && ws && dt0 && nd, "gs_cell3d_split_wgrad: null pointer");
    GS_CHECK_ARG(aligned(dwm, 4) && aligned(w4, 4) && aligned(w6, 4) && aligned(w8, 4) && aligned(softmax3, 4) && aligned(dw4, 4) &&
                     aligned(dw6, 4) && aligned(dw8, 4) && aligned(dots3, 4) && aligned(ws, 4), "gs_cell3d_split_wgrad: misaligned pointer");
    int rc = check_cell_channels("gs_cell3d_split_wgrad", Cin, Cout);
    if (rc) return rc;
    SplitArgs a{};
    a.dwm = dwm; a.w4 = w4; a.w6 = w6; a.w8 = w8; a.sm = softmax3; a.dw4 = dw4; a.dw6 = dw6; a.dw8 = dw8; a.dots = dots3; a.ws = ws;
    GS_CHECK_ARG(split_blocks(Cin, Cout) < 2147483000LL / 3, "gs_cell3d_split_wgrad: too many channels");
    a.gscale = gscale; a.Cin = Cin; a.Cout = Cout; a.nblocks = (int)split_blocks(Cin, Cout);
    for (int i = 0; i < 3; ++i) {
        GS_CHECK_ARG(dt0[i] >= -1 && nd[i] >= 1 && dt0[i] + nd[i] <= 3, "gs_cell3d_split_wgrad: tap box outside -1..2");
        a.dt0[i] = dt0[i]; a.nd[i] = nd[i];
    }
    split_wgrad_kernel<<<a.nblocks, 256, 0, (hipStream_t)stream>>>(a);
    GS_CHECK_LAUNCH("gs_cell3d_split_wgrad");
    split_dots_kernel<<<1, 256, 0, (hipStream_t)stream>>>(a);
    GS_CHECK_LAUNCH("gs_cell3d_split_wgrad");
    return GS_OK;
}

extern "C" int gs_upsample_add3d_fwd(const void* x, void* y, int N, int D, int H, int W, int C, int in_pix_stride, int in_coff,
                                     int out_pix_stride, int out_coff, int dtype, void* stream) {
    int rc = check_upadd("gs_upsample_add3d_fwd", x, y, N, D, H, W, C, in_pix_stride, in_coff, out_pix_stride, out_coff, dtype);
    if (rc) return rc;
    UpAddArgs a{(const unsigned short*)x, (unsigned short*)y, N, D, H, W, C, in_pix_stride, in_coff, out_pix_stride, out_coff};
    const int g = grid_for((int64_t)N * 8 * D * H * W * (C / 32));
    if (dtype == GS_F16) upadd_fwd_kernel<GS_F16><<<g, 256, 0, (hipStream_t)stream>>>(a);
    else upadd_fwd_kernel<GS_BF16><<<g, 256, 0, (hipStream_t)stream>>>(a);
    GS_CHECK_LAUNCH("gs_upsample_add3d_fwd");
    return GS_OK;
}

extern "C" int gs_upsample_add3d_bwd(const void* dy, void* dx, int N, int D, int H, int W, int C, int dy_pix_stride, int dy_coff,
                                     int dx_pix_stride, int dx_coff, int dtype, void* stream) {
    int rc = check_upadd("gs_upsample_add3d_bwd", dx, dy, N, D, H, W, C, dx_pix_stride, dx_coff, dy_pix_stride, dy_coff, dtype);
    if (rc) return rc;
    UpAddArgs a{(const unsigned short*)dy, (unsigned short*)dx, N, D, H, W, C, dx_pix_stride, dx_coff, dy_pix_stride, dy_coff};
    const int g = grid_for((int64_t)N * D * H * W * (C / 32));
    if (dtype == GS_F16) upadd_bwd_kernel<GS_F16><<<g, 256, 0, (hipStream_t)stream>>>(a);
    else upadd_bwd_kernel<GS_BF16><<<g, 256, 0, (hipStream_t)stream>>>(a);
    GS_CHECK_LAUNCH("gs_upsample_add3d_bwd");
    return GS_OK;
}
