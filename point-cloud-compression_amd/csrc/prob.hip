// prob.hip -- AE.ConditionalProbabilityModel (AE.py:87-123) + pn_kit.pmf_to_cdf (pn_kit.py:452-461)
// + torchac's float->16-bit CDF conversion, for a batch of clouds.
//
// Workgroup = one cloud (S decoded patch centres, S % 16 == 0), 4 waves.
//   pass 1: PointNet 3->64->128->256 on every centre tile, max over all S centres -> LDS feature
//   pass 1b: the first Conv's contribution of the 256 feature channels, b0 + W0[:, :256] feat -- the same 512 numbers for every
//           centre of the cloud (AE.py:115-116 concatenates the repeated feature) -- ONCE per cloud, a quarter of the rows per wave,
//           by the same MFMA chain in the same order a centre's column would run (bit-identical to evaluating it per centre,
//           which rounds 1-3 did: 28 % of pass 2's matrix work)
//   pass 2: per tile, Conv 259->512->512->d*L (that vector + the xyz k-tile), logits -> LDS,
//           softmax over L per (centre, latent dim), cumsum, clamp, integer CDF.
// Runs on both sides of the codec from bit-identical centres with a fixed summation order, so the
// encoder's and the decoder's integer CDFs are identical (a range-coder requirement).
#include <math.h>

#include "blobs.h"
#include "common.h"
#include "mfma_chain.h"

// ---- the stages of prob_forward_kernel as functions, for the tiled kernels (pccx_prob_feature, pccx_prob_rows,
// pccx_prob_forward_tiled) at the end of this file: the same statements in the same order, so a centre's chain is prob_forward_kernel's k-tile for k-tile (a column of
// an MFMA tile depends on nothing but its own input column).  prob_forward_kernel itself keeps its own text below: calling these
// from it moved its register allocation (93 against 95 SGPRs, another instruction order), and that kernel is the headline's.
// tests/test_region.py pins the two against each other bit for bit.  bl = the laundered blob pointer of the caller (opaque_uniform).

// pass 1 on one tile: lane (g, n) carries the centre row at xyz; run[] keeps the maxima over the tiles seen so far
__device__ __forceinline__ void prob_pn_tile(const float *bl, const float *xyz, int g, int lane, f32x4 (&run)[16])
{
    f32x4 in[1][1];
    in[0][0][0] = g == 0 ? xyz[0] : 0.f;
    in[0][0][1] = g == 0 ? xyz[1] : 0.f;
    in[0][0][2] = g == 0 ? xyz[2] : 0.f;
    in[0][0][3] = 0.f;
    f32x4 a0[1][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) a0[0][mt] = *(const f32x4 *)(bl + PRB_P_B0 + 16 * mt + 4 * g);
    dense_acc<1, 4, 1, 4>((const f32x4 *)(bl + PRB_P_W0), lane, in, a0);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) a0[0][mt] = relu4(a0[0][mt]);
    f32x4 a1[1][8];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) a1[0][mt] = *(const f32x4 *)(bl + PRB_P_B1 + 16 * mt + 4 * g);
    dense_acc<4, 8, 1, 8>((const f32x4 *)(bl + PRB_P_W1), lane, a0, a1);
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) a1[0][mt] = relu4(a1[0][mt]);
    f32x4 a2[1][16];
#pragma unroll
    for (int mt = 0; mt < 16; ++mt) a2[0][mt] = *(const f32x4 *)(bl + PRB_P_B2 + 16 * mt + 4 * g);
    dense_acc<8, 16, 1, 16>((const f32x4 *)(bl + PRB_P_W2), lane, a1, a2);
#pragma unroll
    for (int mt = 0; mt < 16; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) run[mt][r] = fmaxf(run[mt][r], fmaxf(row16_max(a2[0][mt][r]), 0.f));
}

// pass 1b: u = b0 + W0[:, feature channels] feat, rows 128 wu .. 128 wu + 127 in wave wu (fragments from L2, as pass 1's)
__device__ __forceinline__ void prob_feature_u(const float *bl, const float *sfeat, float *su, int lane, int g, int n, int wu)
{
    f32x4 fin[1][16];
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) fin[0][kt] = *(const f32x4 *)(sfeat + 16 * kt + 4 * g);
    f32x4 u[1][8];
#pragma unroll
    for (int m = 0; m < 8; ++m) u[0][m] = *(const f32x4 *)(bl + PRB_M_B0 + 16 * (8 * wu + m) + 4 * g);
    dense_acc<16, 8, 1, 32>((const f32x4 *)(bl + PRB_M_W0), lane, fin, u, 0, 8 * wu);
    if (n == 0)
#pragma unroll
        for (int m = 0; m < 8; ++m) *(f32x4 *)(su + 16 * (8 * wu + m) + 4 * g) = u[0][m];
}

// pass 2 on one tile: su = pass 1b's 512 numbers in LDS, xyz = this lane's centre row, g from the laundered lane id the caller
// also gave ws.lane; a2 receives the d*L logits of centre n
template <class WS>
__device__ __forceinline__ void prob_mlp_tile(const WS &ws, const float *bl, const float *su, const float *xyz, int g, f32x4 (&a2)[1][8])
{
    int f = 0;
    f32x4 a0[1][32];
#pragma unroll
    for (int mt = 0; mt < 32; ++mt) a0[0][mt] = *(const f32x4 *)(su + 16 * mt + 4 * g);       // bias + the feature k-tiles (pass 1b)
    {
        f32x4 in[1][1];
        in[0][0][0] = g == 0 ? xyz[0] : 0.f;
        in[0][0][1] = g == 0 ? xyz[1] : 0.f;
        in[0][0][2] = g == 0 ? xyz[2] : 0.f;
        in[0][0][3] = 0.f;
        dense_acc_stream<1, 32, 1>(ws, f, in, a0);                                              // the xyz k-tile, last as before
    }
#pragma unroll
    for (int mt = 0; mt < 32; ++mt) a0[0][mt] = relu4(a0[0][mt]);
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) a2[0][mt] = *(const f32x4 *)(bl + PRB_M_B2 + 16 * mt + 4 * g);
#pragma clang loop unroll(full)
    for (int mp = 0; mp < 16; ++mp) {
        f32x4 a1[1][2];
#pragma unroll
        for (int m = 0; m < 2; ++m) a1[0][m] = *(const f32x4 *)(bl + PRB_M_B1 + 16 * (2 * mp + m) + 4 * g);
        dense_acc_stream<32, 2, 1>(ws, f, a0, a1);
#pragma unroll
        for (int m = 0; m < 2; ++m) a1[0][m] = relu4(a1[0][m]);
        dense_acc_stream<2, 8, 1>(ws, f, a1, a2);
    }
}

// softmax + cumsum + integer CDF of the first ncen centres of a tile, one thread per (centre, latent dim); lg = the tile's
// [16][128] logits in LDS, row0 = the output row of its centre 0
__device__ __forceinline__ void prob_tables_tile(const float (*lgt)[128], int lane, int ncen, int d, int L, size_t row0,
                                                 float *__restrict__ pmf, float *__restrict__ cdf, int32_t *__restrict__ cdf_int)
{
    const int Lp = L + 1;
    for (int e = lane; e < ncen * d; e += 64) {
        const int cn = e / d, i = e % d;
        const float *lg = &lgt[cn][i * L];              // output.view(B,S,d,L): channel i*L + l
        float mx = -INFINITY;
        for (int l = 0; l < L; ++l) mx = fmaxf(mx, lg[l]);
        float sum = 0.f;
        for (int l = 0; l < L; ++l) sum += expf(lg[l] - mx);
        const size_t row = (row0 + cn) * d + i;
        float run_c = 0.f;
        if (cdf) cdf[row * Lp] = 0.f;
        if (cdf_int) cdf_int[row * Lp] = 0;
        for (int l = 0; l < L; ++l) {
            const float pv = expf(lg[l] - mx) / sum;
            if (pmf) pmf[row * L + l] = pv;
            run_c = run_c + pv;                                        // cumsum (pn_kit.py:453)
            const float cv = fminf(run_c, 1.0f);                       // clamp(max=1) (pn_kit.py:460)
            if (cdf) cdf[row * Lp + l + 1] = cv;
            // torchac: round(cdf * (2^16 - (Lp-1))) + arange(Lp), kept to 16 bits
            if (cdf_int) cdf_int[row * Lp + l + 1] = ((int)rintf(cv * (float)(65536 - (Lp - 1))) + (l + 1)) & 0xFFFF;
        }
    }
}

__global__ __launch_bounds__(256, 2) void prob_forward_kernel(const float *__restrict__ centres, int S, int d, int L,
                                                              const float *__restrict__ blob, float *__restrict__ pmf,
                                                              float *__restrict__ cdf, int32_t *__restrict__ cdf_int)
{
    __shared__ __attribute__((aligned(16))) f32x4 swt[4 * PRB_WS_CHUNK * 64];   // 32 KiB weight ring, four chunks deep
    __shared__ __attribute__((aligned(16))) float sfeat[256];
    __shared__ __attribute__((aligned(16))) float su[512];
    __shared__ float smax[4][256];
    __shared__ __attribute__((aligned(16))) float slog[4][16][128];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, n = lane & 15;
    const size_t b = blockIdx.x;
    const float *cp = centres + b * (size_t)S * 3;
    const int ntiles = S >> 4;
    const int wu = __builtin_amdgcn_readfirstlane(w);
    WStreamT<PRB_WS_CHUNK, 4, 4> ws{blob + PRB_STREAM, swt, PRB_STREAM_CHUNKS, lane, wu, true};
    ws.prologue();                                        // the first chunks of model_mlp arrive while model_pn runs

    // ---- pass 1: model_pn (AE.py:96,112)
    f32x4 run[16];
#pragma unroll
    for (int mt = 0; mt < 16; ++mt) run[mt][0] = run[mt][1] = run[mt][2] = run[mt][3] = -INFINITY;
    for (int tile = w; tile < ntiles; tile += 4) {
        const float *bl = opaque_uniform(blob);
        const int c = tile * 16 + n;
        f32x4 in[1][1];
        in[0][0][0] = g == 0 ? cp[3 * c] : 0.f;
        in[0][0][1] = g == 0 ? cp[3 * c + 1] : 0.f;
        in[0][0][2] = g == 0 ? cp[3 * c + 2] : 0.f;
        in[0][0][3] = 0.f;
        f32x4 a0[1][4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) a0[0][mt] = *(const f32x4 *)(bl + PRB_P_B0 + 16 * mt + 4 * g);
        dense_acc<1, 4, 1, 4>((const f32x4 *)(bl + PRB_P_W0), lane, in, a0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) a0[0][mt] = relu4(a0[0][mt]);
        f32x4 a1[1][8];
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) a1[0][mt] = *(const f32x4 *)(bl + PRB_P_B1 + 16 * mt + 4 * g);
        dense_acc<4, 8, 1, 8>((const f32x4 *)(bl + PRB_P_W1), lane, a0, a1);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) a1[0][mt] = relu4(a1[0][mt]);
        f32x4 a2[1][16];
#pragma unroll
        for (int mt = 0; mt < 16; ++mt) a2[0][mt] = *(const f32x4 *)(bl + PRB_P_B2 + 16 * mt + 4 * g);
        dense_acc<8, 16, 1, 16>((const f32x4 *)(bl + PRB_P_W2), lane, a1, a2);
#pragma unroll
        for (int mt = 0; mt < 16; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) run[mt][r] = fmaxf(run[mt][r], fmaxf(row16_max(a2[0][mt][r]), 0.f));
    }
    if (n == 0)
#pragma unroll
        for (int mt = 0; mt < 16; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) smax[w][16 * mt + 4 * g + r] = run[mt][r];
    __syncthreads();
    sfeat[tid] = fmaxf(fmaxf(smax[0][tid], smax[1][tid]), fmaxf(smax[2][tid], smax[3][tid]));
    __syncthreads();

    // ---- pass 1b: u = b0 + W0[:, feature channels] feat, rows 128 w .. 128 w + 127 in wave w (fragments from L2, as pass 1's)
    {
        const float *bl = opaque_uniform(blob);
        f32x4 fin[1][16];
#pragma unroll
        for (int kt = 0; kt < 16; ++kt) fin[0][kt] = *(const f32x4 *)(sfeat + 16 * kt + 4 * g);
        f32x4 u[1][8];
#pragma unroll
        for (int m = 0; m < 8; ++m) u[0][m] = *(const f32x4 *)(bl + PRB_M_B0 + 16 * (8 * wu + m) + 4 * g);
        dense_acc<16, 8, 1, 32>((const f32x4 *)(bl + PRB_M_W0), lane, fin, u, 0, 8 * wu);
        if (n == 0)
#pragma unroll
            for (int m = 0; m < 8; ++m) *(f32x4 *)(su + 16 * (8 * wu + m) + 4 * g) = u[0][m];
    }
    __syncthreads();

    // ---- pass 2: model_mlp (AE.py:97-105,115-118) + softmax (AE.py:120) + cdf
    const int Lp = L + 1;
    for (int tile0 = 0; tile0 < ntiles; tile0 += 4) {
        const int tile = tile0 + w;
        {
            // All four waves walk the same weight sequence on their own tile (an idle wave of the last round walks it on a
            // clamped tile and discards the result: the ring's barriers need every wave), streamed L2 -> LDS three chunks ahead.
            const float *bl = opaque_uniform(blob);
            ws.g = bl + PRB_STREAM;
            // this pass's lane indices from a laundered lane id: nothing computed for pass 1 or for the softmax below is carried through
            // the 160 accumulator registers of the two wide layers (round 3: ten values spilled to scratch around them)
            int lane2 = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            asm volatile("" : "+v"(lane2));
            const int g = lane2 >> 4, n = lane2 & 15;
            ws.lane = lane2;
            const int c = (tile < ntiles ? tile : ntiles - 1) * 16 + n;
            int f = 0;
            f32x4 a0[1][32];
#pragma unroll
            for (int mt = 0; mt < 32; ++mt) a0[0][mt] = *(const f32x4 *)(su + 16 * mt + 4 * g);       // bias + the feature k-tiles (pass 1b)
            {
                f32x4 in[1][1];
                in[0][0][0] = g == 0 ? cp[3 * c] : 0.f;
                in[0][0][1] = g == 0 ? cp[3 * c + 1] : 0.f;
                in[0][0][2] = g == 0 ? cp[3 * c + 2] : 0.f;
                in[0][0][3] = 0.f;
                dense_acc_stream<1, 32, 1>(ws, f, in, a0);                                              // the xyz k-tile, last as before
            }
#pragma unroll
            for (int mt = 0; mt < 32; ++mt) a0[0][mt] = relu4(a0[0][mt]);
            f32x4 a2[1][8];
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) a2[0][mt] = *(const f32x4 *)(bl + PRB_M_B2 + 16 * mt + 4 * g);
#pragma clang loop unroll(full)
            for (int mp = 0; mp < 16; ++mp) {
                f32x4 a1[1][2];
#pragma unroll
                for (int m = 0; m < 2; ++m) a1[0][m] = *(const f32x4 *)(bl + PRB_M_B1 + 16 * (2 * mp + m) + 4 * g);
                dense_acc_stream<32, 2, 1>(ws, f, a0, a1);
#pragma unroll
                for (int m = 0; m < 2; ++m) a1[0][m] = relu4(a1[0][m]);
                dense_acc_stream<2, 8, 1>(ws, f, a1, a2);
            }
            if (tile < ntiles)
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) *(f32x4 *)(&slog[w][n][16 * mt + 4 * g]) = a2[0][mt];
        }
        __syncthreads();
        // one thread per (centre, latent dim): the wave's own tile, 16 centres x 16 dims
        if (tile < ntiles) {
            for (int e = lane; e < 16 * d; e += 64) {
                const int cn = e / d, i = e % d;
                const float *lg = &slog[w][cn][i * L];          // output.view(B,S,d,L): channel i*L + l
                float mx = -INFINITY;
                for (int l = 0; l < L; ++l) mx = fmaxf(mx, lg[l]);
                float sum = 0.f;
                for (int l = 0; l < L; ++l) sum += expf(lg[l] - mx);
                const size_t row = (b * S + (size_t)tile * 16 + cn) * d + i;
                float run_c = 0.f;
                if (cdf) cdf[row * Lp] = 0.f;
                if (cdf_int) cdf_int[row * Lp] = 0;
                for (int l = 0; l < L; ++l) {
                    const float pv = expf(lg[l] - mx) / sum;
                    if (pmf) pmf[row * L + l] = pv;
                    run_c = run_c + pv;                                        // cumsum (pn_kit.py:453)
                    const float cv = fminf(run_c, 1.0f);                       // clamp(max=1) (pn_kit.py:460)
                    if (cdf) cdf[row * Lp + l + 1] = cv;
                    // torchac: round(cdf * (2^16 - (Lp-1))) + arange(Lp), kept to 16 bits
                    if (cdf_int) cdf_int[row * Lp + l + 1] = ((int)rintf(cv * (float)(65536 - (Lp - 1))) + (l + 1)) & 0xFFFF;
                }
            }
        }
        __syncthreads();
    }
    ws.drain();                                           // no DMA may land after the workgroup retires
}

// ---- the table stage of prob_forward_distinct_kernel: a wave copies the rows of every centre of its cloud from the centre's slot.
// rows = the wave's [16][128] floats (pmf, later the clamped cumsum, of the tile's slots), slots = centre -> slot.  The lanes share out
// (centre, W consecutive words of its row): a centre's row is contiguous in the output, so W = 4 is one 16-byte store per lane
// (row length a multiple of 4 and the array 16-byte aligned; W = 1 otherwise).
__device__ __forceinline__ void prob_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int W>
__device__ __forceinline__ void prob_store_pmf(const float *rows, const int *slots, int nslots, int t, int lane, size_t row0, int rl,
                                               float *__restrict__ pmf)
{
    const int per = rl / W;
    for (int it = lane; it < nslots * per; it += 64) {
        const int c = it / per, j = (it % per) * W, sl = slots[c];
        if ((sl >> 4) != t) continue;
        const float *src = rows + (sl & 15) * 128 + j;
        float *dst = pmf + (row0 + c) * (size_t)rl + j;
        if constexpr (W == 4) *(f32x4 *)dst = *(const f32x4 *)src;
        else *dst = *src;
    }
}

template <int W>
__device__ __forceinline__ void prob_store_cdf(const float *rows, const int *slots, int nslots, int t, int lane, size_t row0, int d, int L,
                                               float *__restrict__ cdf, int32_t *__restrict__ cdf_int)
{
    const int Lp = L + 1, rl = d * Lp, per = rl / W;
    for (int it = lane; it < nslots * per; it += 64) {
        const int c = it / per, j = (it % per) * W, sl = slots[c];
        if ((sl >> 4) != t) continue;
        float cv[W];
        int ci[W];
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const int i = (j + q) / Lp, l = (j + q) % Lp;                          // level 0 of a row is the leading zero
            cv[q] = l ? rows[(sl & 15) * 128 + i * L + l - 1] : 0.f;
            // torchac: round(cdf * (2^16 - (Lp-1))) + arange(Lp), kept to 16 bits
            ci[q] = l ? ((int)rintf(cv[q] * (float)(65536 - (Lp - 1))) + l) & 0xFFFF : 0;
        }
        const size_t o = (row0 + c) * (size_t)rl + j;
        if constexpr (W == 4) {
            if (cdf) *(f32x4 *)(cdf + o) = f32x4{cv[0], cv[1], cv[2], cv[3]};
            if (cdf_int) *(int4 *)(cdf_int + o) = make_int4(ci[0], ci[1], ci[2], ci[3]);
        } else {
            if (cdf) cdf[o] = cv[0];
            if (cdf_int) cdf_int[o] = ci[0];
        }
    }
}

// ------------------------------------------------------------------------------------------
// The same function for clouds whose centres repeat (octree_mode "reference": at most 8 distinct rows among a cloud's 64).  A column of
// an MFMA tile depends on nothing but its own input column, and pass 1's maximum is the same over the distinct centres as over all of
// them, so every distinct centre row is evaluated once and its tables are copied to the duplicates: bit for bit prob_forward_kernel's
// outputs.
// Workgroup = FOUR clouds, one per wave (a wave past the batch walks the last cloud and writes nothing: the ring's barriers need it).
//   distinct: lane c holds centre c (S <= 64); rows are compared bit for bit, the representative is the first equal row and its slot its
//             rank among the representatives; slot -> centre and centre -> slot go to LDS.  Slots past the last one read centre 0.
//   pass 1 : as above on tiles of 16 slots, all of the wave's own
//   pass 1b: once per workgroup -- column n of the B operand carries cloud (n & 3)'s feature, a quarter of the 512 rows per wave
//   pass 2 : tiles of 16 slots; the loop count is the workgroup's largest (a wave with fewer tiles walks its last one again)
//   tables : softmax once per (slot, latent dim), in place over the logits, then the pmf rows of every centre of the tile's slots are
//            copied out; the cumsum + clamp again in place, then the cdf / cdf_int rows (the integer CDF is a function of the clamped
//            value and the level alone).  One expf pair per distinct (centre, dim, level) instead of per centre.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void prob_forward_distinct_kernel(const float *__restrict__ centres, int B, int S, int d, int L,
                                                                       const float *__restrict__ blob, float *__restrict__ pmf,
                                                                       float *__restrict__ cdf, int32_t *__restrict__ cdf_int)
{
    __shared__ __attribute__((aligned(16))) f32x4 swt[4 * PRB_WS_CHUNK * 64];   // 32 KiB weight ring, four chunks deep
    __shared__ __attribute__((aligned(16))) float sfeat[4][256];
    __shared__ __attribute__((aligned(16))) float su[4][512];
    __shared__ __attribute__((aligned(16))) float slog[4][16][128];
    __shared__ int slot_of[4][64], cen_of[4][64], s_nt[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const int bw = blockIdx.x * 4 + wu;
    const bool live = bw < B;
    const size_t b = live ? bw : B - 1;
    const float *cp = centres + b * (size_t)S * 3;
    WStreamT<PRB_WS_CHUNK, 4, 4> ws{blob + PRB_STREAM, swt, PRB_STREAM_CHUNKS, lane, wu, true};
    ws.prologue();                                        // the first chunks of model_mlp arrive while model_pn runs

    // ---- the distinct centres of this wave's cloud
    int nt;
    {
        const bool valid = lane < S;
        const int cl = valid ? lane : S - 1;
        const unsigned kx = __float_as_uint(cp[3 * cl]), ky = __float_as_uint(cp[3 * cl + 1]), kz = __float_as_uint(cp[3 * cl + 2]);
        int rep = cl;
        for (int j = S - 1; j >= 0; --j) {                // descending: the first equal row is the one that stays
            const unsigned jx = __builtin_amdgcn_readlane(kx, j), jy = __builtin_amdgcn_readlane(ky, j), jz = __builtin_amdgcn_readlane(kz, j);
            if (jx == kx && jy == ky && jz == kz) rep = j;
        }
        const unsigned long long reps = __ballot(valid && rep == lane);
        const int rank = __popcll(reps & ((1ull << lane) - 1ull));
        const int slot = __shfl(rank, rep);
        // slot -> centre in ONE store per lane, so no order between stores is relied on: lane s < n_distinct takes the s-th set bit of
        // the representatives' mask (slots are ranks, so that lane is the slot's centre), the other slots read centre 0
        {
            unsigned long long m = reps;
            const int nd = __popcll(reps);
            for (int i = 0; i < (lane < nd ? lane : 0); ++i) m &= m - 1ull;
            cen_of[w][lane] = lane < nd ? __ffsll((long long)m) - 1 : 0;
        }
        if (valid) slot_of[w][lane] = slot;
        nt = __builtin_amdgcn_readfirstlane((__popcll(reps) + 15) >> 4);
        if (lane == 0) s_nt[w] = nt;
    }
    __syncthreads();

    // ---- pass 1: model_pn (AE.py:96,112) over the wave's own slots
    {
        f32x4 run[16];
#pragma unroll
        for (int mt = 0; mt < 16; ++mt) run[mt][0] = run[mt][1] = run[mt][2] = run[mt][3] = -INFINITY;
        for (int tile = 0; tile < nt; ++tile) {
            const float *bl = opaque_uniform(blob);
            const int c = cen_of[w][tile * 16 + n];
            f32x4 in[1][1];
            in[0][0][0] = g == 0 ? cp[3 * c] : 0.f;
            in[0][0][1] = g == 0 ? cp[3 * c + 1] : 0.f;
            in[0][0][2] = g == 0 ? cp[3 * c + 2] : 0.f;
            in[0][0][3] = 0.f;
            f32x4 a0[1][4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a0[0][mt] = *(const f32x4 *)(bl + PRB_P_B0 + 16 * mt + 4 * g);
            dense_acc<1, 4, 1, 4>((const f32x4 *)(bl + PRB_P_W0), lane, in, a0);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a0[0][mt] = relu4(a0[0][mt]);
            f32x4 a1[1][8];
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) a1[0][mt] = *(const f32x4 *)(bl + PRB_P_B1 + 16 * mt + 4 * g);
            dense_acc<4, 8, 1, 8>((const f32x4 *)(bl + PRB_P_W1), lane, a0, a1);
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) a1[0][mt] = relu4(a1[0][mt]);
            f32x4 a2[1][16];
#pragma unroll
            for (int mt = 0; mt < 16; ++mt) a2[0][mt] = *(const f32x4 *)(bl + PRB_P_B2 + 16 * mt + 4 * g);
            dense_acc<8, 16, 1, 16>((const f32x4 *)(bl + PRB_P_W2), lane, a1, a2);
#pragma unroll
            for (int mt = 0; mt < 16; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) run[mt][r] = fmaxf(run[mt][r], fmaxf(row16_max(a2[0][mt][r]), 0.f));
        }
        if (n == 0)
#pragma unroll
            for (int mt = 0; mt < 16; ++mt) *(f32x4 *)(&sfeat[w][16 * mt + 4 * g]) = run[mt];
    }
    __syncthreads();
    const int ntmax = max(max(s_nt[0], s_nt[1]), max(s_nt[2], s_nt[3]));

    // ---- pass 1b: u = b0 + W0[:, feature channels] feat for the four clouds at once: column n is cloud n & 3, rows 128 w .. 128 w + 127
    {
        const float *bl = opaque_uniform(blob);
        f32x4 fin[1][16];
#pragma unroll
        for (int kt = 0; kt < 16; ++kt) fin[0][kt] = *(const f32x4 *)(&sfeat[n & 3][16 * kt + 4 * g]);
        f32x4 u[1][8];
#pragma unroll
        for (int m = 0; m < 8; ++m) u[0][m] = *(const f32x4 *)(bl + PRB_M_B0 + 16 * (8 * wu + m) + 4 * g);
        dense_acc<16, 8, 1, 32>((const f32x4 *)(bl + PRB_M_W0), lane, fin, u, 0, 8 * wu);
        if (n < 4)
#pragma unroll
            for (int m = 0; m < 8; ++m) *(f32x4 *)(&su[n][16 * (8 * wu + m) + 4 * g]) = u[0][m];
    }
    __syncthreads();

    // ---- pass 2: model_mlp (AE.py:97-105,115-118) on tiles of slots, then the tables of every centre
    const int Lp = L + 1;
    for (int t = 0; t < ntmax; ++t) {
        const bool act = live && t < nt;                  // wave-uniform
        {
            const float *bl = opaque_uniform(blob);
            ws.g = bl + PRB_STREAM;
            // lane indices from a laundered lane id, as in prob_forward_kernel: nothing is carried through the wide layers' accumulators
            int lane2 = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            asm volatile("" : "+v"(lane2));
            const int g = lane2 >> 4, n = lane2 & 15;
            ws.lane = lane2;
            const int c = cen_of[wu][(t < nt ? t : nt - 1) * 16 + n];
            int f = 0;
            f32x4 a0[1][32];
#pragma unroll
            for (int mt = 0; mt < 32; ++mt) a0[0][mt] = *(const f32x4 *)(&su[wu][16 * mt + 4 * g]);   // bias + the feature k-tiles (pass 1b)
            {
                f32x4 in[1][1];
                in[0][0][0] = g == 0 ? cp[3 * c] : 0.f;
                in[0][0][1] = g == 0 ? cp[3 * c + 1] : 0.f;
                in[0][0][2] = g == 0 ? cp[3 * c + 2] : 0.f;
                in[0][0][3] = 0.f;
                dense_acc_stream<1, 32, 1>(ws, f, in, a0);                                              // the xyz k-tile, last as before
            }
#pragma unroll
            for (int mt = 0; mt < 32; ++mt) a0[0][mt] = relu4(a0[0][mt]);
            f32x4 a2[1][8];
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) a2[0][mt] = *(const f32x4 *)(bl + PRB_M_B2 + 16 * mt + 4 * g);
#pragma clang loop unroll(full)
            for (int mp = 0; mp < 16; ++mp) {
                f32x4 a1[1][2];
#pragma unroll
                for (int m = 0; m < 2; ++m) a1[0][m] = *(const f32x4 *)(bl + PRB_M_B1 + 16 * (2 * mp + m) + 4 * g);
                dense_acc_stream<32, 2, 1>(ws, f, a0, a1);
#pragma unroll
                for (int m = 0; m < 2; ++m) a1[0][m] = relu4(a1[0][m]);
                dense_acc_stream<2, 8, 1>(ws, f, a1, a2);
            }
            if (t < nt)
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) *(f32x4 *)(&slog[wu][n][16 * mt + 4 * g]) = a2[0][mt];
        }
        // From here to the end of the tile a wave touches its own slog / slot_of only: LDS operations of one wave complete in order, so
        // a wave-local fence (prob_wave_sync) orders the phases and the four clouds of the workgroup do not wait for each other.
        prob_wave_sync();
        // softmax, one thread per (slot, latent dim) of the tile, in place: the L logits of the pair become its pmf
        const int nslots = S < 64 ? S : 64;               // slot_of / cen_of entries of this cloud
        if (act)
            for (int e = lane; e < 16 * d; e += 64) {
                float *lg = &slog[wu][e / d][(e % d) * L];      // output.view(B,S,d,L): channel i*L + l
                float mx = -INFINITY;
                for (int l = 0; l < L; ++l) mx = fmaxf(mx, lg[l]);
                float sum = 0.f;
                for (int l = 0; l < L; ++l) sum += expf(lg[l] - mx);
                for (int l = 0; l < L; ++l) lg[l] = expf(lg[l] - mx) / sum;
            }
        prob_wave_sync();
        if (act && pmf) {
            if ((d * L) % 4 == 0 && ((uintptr_t)pmf & 15) == 0) prob_store_pmf<4>(&slog[wu][0][0], slot_of[wu], nslots, t, lane, b * S, d * L, pmf);
            else prob_store_pmf<1>(&slog[wu][0][0], slot_of[wu], nslots, t, lane, b * S, d * L, pmf);
        }
        if (cdf || cdf_int) {
            prob_wave_sync();
            if (act)
                for (int e = lane; e < 16 * d; e += 64) {
                    float *lg = &slog[wu][e / d][(e % d) * L];
                    float run_c = 0.f;
                    for (int l = 0; l < L; ++l) {
                        run_c = run_c + lg[l];                                     // cumsum (pn_kit.py:453)
                        lg[l] = fminf(run_c, 1.0f);                                // clamp(max=1) (pn_kit.py:460)
                    }
                }
            prob_wave_sync();
            if (act) {
                if ((d * Lp) % 4 == 0 && (((uintptr_t)cdf | (uintptr_t)cdf_int) & 15) == 0)
                    prob_store_cdf<4>(&slog[wu][0][0], slot_of[wu], nslots, t, lane, b * S, d, L, cdf, cdf_int);
                else
                    prob_store_cdf<1>(&slog[wu][0][0], slot_of[wu], nslots, t, lane, b * S, d, L, cdf, cdf_int);
            }
        }
        prob_wave_sync();
    }
    ws.drain();                                           // no DMA may land after the workgroup retires
}

extern "C" int pccx_prob_forward(const float *centres, int B, int S, int d, int L, const float *prob_blob, float *pmf,
                                 float *cdf, int32_t *cdf_int, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    PCCX_CHECK_ARG(centres && prob_blob, "pccx_prob_forward: null pointer");
    PCCX_CHECK_ARG(pmf || cdf || cdf_int, "pccx_prob_forward: no output requested");
    PCCX_CHECK_ARG(B >= 0 && S >= 16 && S % 16 == 0, "pccx_prob_forward: need S %% 16 == 0 (S=%d)", S);
    PCCX_CHECK_ARG(d >= 1 && d <= 16 && L >= 1 && L <= 15 && d * L <= 128, "pccx_prob_forward: unsupported d=%d L=%d", d, L);
    hipLaunchKernelGGL(prob_forward_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, centres, S, d, L, prob_blob, pmf, cdf,
                       cdf_int);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

extern "C" int pccx_prob_forward_distinct(const float *centres, int B, int S, int d, int L, const float *prob_blob, float *pmf,
                                          float *cdf, int32_t *cdf_int, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    PCCX_CHECK_ARG(centres && prob_blob, "pccx_prob_forward_distinct: null pointer");
    PCCX_CHECK_ARG(pmf || cdf || cdf_int, "pccx_prob_forward_distinct: no output requested");
    PCCX_CHECK_ARG(B >= 0 && S >= 16 && S % 16 == 0 && S <= 64, "pccx_prob_forward_distinct: need S %% 16 == 0, S <= 64 (S=%d)", S);
    PCCX_CHECK_ARG(d >= 1 && d <= 16 && L >= 1 && L <= 15 && d * L <= 128, "pccx_prob_forward_distinct: unsupported d=%d L=%d", d, L);
    hipLaunchKernelGGL(prob_forward_distinct_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, centres, B, S, d, L, prob_blob,
                       pmf, cdf, cdf_int);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

// ------------------------------------------------------------------------------------------
// The same function cut at the one quantity that couples a cloud's centres, pass 1's maximum, so that a cloud's tiles are dealt
// over the chip.  prob_forward_kernel gives a cloud to ONE workgroup, which is right for 1024 clouds of 64
// centres and leaves 255 CUs idle for one cloud of 8192.  Two users: region decode (pccx_prob_feature + pccx_prob_rows: one cloud,
// a LIST of its rows) and the opt-in whole-cloud path Codec(prob_path="tiles") (pccx_prob_forward_tiled: a batch, every row).
// The cloud is blockIdx.y in all three kernels; launches follow in stream order: no cooperative launch, no flag, no spin.
//   prob_feature_partial_kernel, grid (nwg, B): pass 1 with the cloud's 16-centre tiles dealt over up to 64 workgroups x 4 waves;
//       each workgroup leaves its 256 maxima (over its four waves) in partial[b][wg][256].  fmaxf is exact in any grouping, so the
//       maximum over the partials is prob_forward_kernel's sfeat[] bit for bit (the -INFINITY start and the fmaxf(., 0) stay as
//       there).  A wave that gets no tile leaves -INFINITY, which no fmaxf keeps (every cloud has a tile).
//   prob_feature_reduce_kernel, grid (1, B): one workgroup takes that maximum and runs pass 1b with prob_forward_kernel's own call
//       and wave split; the 512 numbers su[] go to feature[b][512] in HBM.
//   prob_rows_kernel<LIST>, grid (ceil(rows / 64), B): pass 2 + softmax + tables.  A wave takes 16 rows, a workgroup four tiles in
//       ONE pass over the weight ring; all four waves walk every chunk, an idle wave of the last workgroup on a clamped tile whose
//       result it drops, and ws.drain() runs before the workgroup retires.
//       LIST = false: row r is centre r of the cloud (S % 16 == 0: no ragged tile), all three outputs.
//       LIST = true : compact row r stands for row seg_idx[r / G] * G + r % G of the cloud (clamped into [0, S - 1]: the rows past S
//       of a ragged last segment are computed on row S - 1 and never read); cdf_int alone, compact.  A compile-time branch: it sits
//       in the wave's address computation in front of a 220-VGPR body.
// ------------------------------------------------------------------------------------------
#define PRB_FEATURE_MAX_WG 64
#define PRB_TILED_MAX_B 65535                             // gridDim.y

__global__ __launch_bounds__(256, 2) void prob_feature_partial_kernel(const float *__restrict__ centres, int S,
                                                                      const float *__restrict__ blob, float *__restrict__ partial)
{
    __shared__ float smax[4][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int ntiles = S >> 4;
    const float *cp = centres + (size_t)blockIdx.y * S * 3;
    f32x4 run[16];
#pragma unroll
    for (int mt = 0; mt < 16; ++mt) run[mt][0] = run[mt][1] = run[mt][2] = run[mt][3] = -INFINITY;
    for (int tile = blockIdx.x * 4 + w; tile < ntiles; tile += 4 * gridDim.x) {
        const float *bl = opaque_uniform(blob);
        prob_pn_tile(bl, cp + 3 * (tile * 16 + n), g, lane, run);
    }
    if (n == 0)
#pragma unroll
        for (int mt = 0; mt < 16; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) smax[w][16 * mt + 4 * g + r] = run[mt][r];
    __syncthreads();
    partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid] =
        fmaxf(fmaxf(smax[0][tid], smax[1][tid]), fmaxf(smax[2][tid], smax[3][tid]));
}

__global__ __launch_bounds__(256, 2) void prob_feature_reduce_kernel(const float *__restrict__ partial, int nwg,
                                                                     const float *__restrict__ blob, float *__restrict__ feature)
{
    __shared__ __attribute__((aligned(16))) float sfeat[256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const float *pp = partial + (size_t)blockIdx.y * nwg * 256;
    float m = pp[tid];
    for (int j = 1; j < nwg; ++j) m = fmaxf(m, pp[(size_t)j * 256 + tid]);
    sfeat[tid] = m;
    __syncthreads();
    prob_feature_u(opaque_uniform(blob), sfeat, feature + (size_t)blockIdx.y * 512, lane, g, n, wu);
}

template <bool LIST>
__global__ __launch_bounds__(256, 2) void prob_rows_kernel(const float *__restrict__ centres, int S, int d, int L,
                                                           const float *__restrict__ blob, const float *__restrict__ feature,
                                                           const int32_t *__restrict__ seg_idx, int n_seg, int G,
                                                           float *__restrict__ pmf, float *__restrict__ cdf,
                                                           int32_t *__restrict__ cdf_int)
{
    __shared__ __attribute__((aligned(16))) f32x4 swt[4 * PRB_WS_CHUNK * 64];   // 32 KiB weight ring, four chunks deep
    __shared__ __attribute__((aligned(16))) float su[512];
    __shared__ __attribute__((aligned(16))) float slog[4][16][128];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const int nrows = LIST ? n_seg * G : S, ntiles = (nrows + 15) >> 4;
    const size_t b = blockIdx.y;
    WStreamT<PRB_WS_CHUNK, 4, 4> ws{blob + PRB_STREAM, swt, PRB_STREAM_CHUNKS, lane, wu, false};   // one pass: nothing is issued past it
    ws.prologue();
    if (tid < 128) *(f32x4 *)(su + 4 * tid) = *(const f32x4 *)(feature + b * 512 + 4 * tid);
    __syncthreads();

    const int tile = blockIdx.x * 4 + w;
    {
        const float *bl = opaque_uniform(blob);
        ws.g = bl + PRB_STREAM;
        // lane indices from a laundered lane id, as in prob_forward_kernel
        int lane2 = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        asm volatile("" : "+v"(lane2));
        const int g = lane2 >> 4, n = lane2 & 15;
        ws.lane = lane2;
        int c = (tile < ntiles ? tile : ntiles - 1) * 16 + n;
        if (LIST) {
            const int r = c < nrows ? c : nrows - 1;              // the ragged last tile: walked on its last row, not stored
            c = seg_idx[r / G] * G + r % G;
            c = c < 0 ? 0 : (c < S ? c : S - 1);                  // whatever the list holds, the address stays inside the cloud
        }
        f32x4 a2[1][8];
        prob_mlp_tile(ws, bl, su, centres + (b * S + c) * 3, g, a2);
        if (tile < ntiles)
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) *(f32x4 *)(&slog[w][n][16 * mt + 4 * g]) = a2[0][mt];
    }
    __syncthreads();
    if (tile < ntiles) {
        const int left = nrows - tile * 16;
        prob_tables_tile(slog[w], lane, LIST && left < 16 ? left : 16, d, L, (LIST ? 0 : b * S) + (size_t)tile * 16,
                         LIST ? nullptr : pmf, LIST ? nullptr : cdf, cdf_int);
    }
    ws.drain();                                           // no DMA may land after the workgroup retires
}

static int prob_feature_workgroups(int S)
{
    const int rounds = ((S >> 4) + 3) / 4;                // workgroup rounds of four tiles
    return rounds < 1 ? 1 : (rounds > PRB_FEATURE_MAX_WG ? PRB_FEATURE_MAX_WG : rounds);
}

// pass 1 + 1b of B clouds: partial[B][nwg][256] -> feature[B][512]
static int prob_feature_launch(const float *centres, int B, int S, const float *prob_blob, float *partial, float *feature, hipStream_t stream)
{
    const int nwg = prob_feature_workgroups(S);
    hipLaunchKernelGGL(prob_feature_partial_kernel, dim3(nwg, B), dim3(256), 0, stream, centres, S, prob_blob, partial);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(prob_feature_reduce_kernel, dim3(1, B), dim3(256), 0, stream, partial, nwg, prob_blob, feature);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

extern "C" size_t pccx_prob_feature_workspace_floats(int S)
{
    return S < 16 ? 0 : (size_t)prob_feature_workgroups(S) * 256;
}

extern "C" int pccx_prob_feature(const float *centres, int S, const float *prob_blob, float *workspace, float *feature, void *stream)
{
    PCCX_CHECK_ARG(centres && prob_blob && workspace && feature, "pccx_prob_feature: null pointer");
    PCCX_CHECK_ARG(S >= 16 && S % 16 == 0, "pccx_prob_feature: need S %% 16 == 0 (S=%d)", S);
    PCCX_CHECK_ARG(((uintptr_t)feature & 15) == 0, "pccx_prob_feature: feature must be 16-byte aligned");
    return prob_feature_launch(centres, 1, S, prob_blob, workspace, feature, (hipStream_t)stream);
}

extern "C" int pccx_prob_rows(const float *centres, int S, int d, int L, const float *prob_blob, const float *feature,
                              const int32_t *seg_idx, int n_seg, int G, int32_t *cdf_int, void *stream)
{
    if (n_seg == 0) return PCCX_OK;   // empty list: nothing to do, pointers may be null
    PCCX_CHECK_ARG(centres && prob_blob && feature && seg_idx && cdf_int, "pccx_prob_rows: null pointer");
    PCCX_CHECK_ARG(S >= 16 && S % 16 == 0, "pccx_prob_rows: need S %% 16 == 0 (S=%d)", S);
    PCCX_CHECK_ARG(d >= 1 && d <= 16 && L >= 1 && L <= 15 && d * L <= 128, "pccx_prob_rows: unsupported d=%d L=%d", d, L);
    PCCX_CHECK_ARG(G >= 1 && n_seg >= 0 && n_seg <= (S + G - 1) / G, "pccx_prob_rows: %d segments of G=%d patches listed for S=%d", n_seg, G, S);
    PCCX_CHECK_ARG(((uintptr_t)feature & 15) == 0, "pccx_prob_rows: feature must be 16-byte aligned");
    const int ntiles = (int)(((int64_t)n_seg * G + 15) >> 4);
    hipLaunchKernelGGL(prob_rows_kernel<true>, dim3((ntiles + 3) / 4), dim3(256), 0, (hipStream_t)stream, centres, S, d, L, prob_blob,
                       feature, seg_idx, n_seg, G, (float *)nullptr, (float *)nullptr, cdf_int);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

extern "C" size_t pccx_prob_forward_tiled_workspace_floats(int B, int S)
{
    if (B < 1 || S < 16) return 0;
    return (size_t)B * ((size_t)prob_feature_workgroups(S) * 256 + 512);      // the partial maxima, then 512 floats per cloud
}

extern "C" int pccx_prob_forward_tiled(const float *centres, int B, int S, int d, int L, const float *prob_blob, float *pmf,
                                       float *cdf, int32_t *cdf_int, float *workspace, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    PCCX_CHECK_ARG(centres && prob_blob && workspace, "pccx_prob_forward_tiled: null pointer");
    PCCX_CHECK_ARG(pmf || cdf || cdf_int, "pccx_prob_forward_tiled: no output requested");
    PCCX_CHECK_ARG(B >= 0 && B <= PRB_TILED_MAX_B, "pccx_prob_forward_tiled: need 0 <= B <= %d, the grid's second dimension (B=%d)",
                   PRB_TILED_MAX_B, B);
    PCCX_CHECK_ARG(S >= 16 && S % 16 == 0, "pccx_prob_forward_tiled: need S %% 16 == 0 (S=%d)", S);
    PCCX_CHECK_ARG(d >= 1 && d <= 16 && L >= 1 && L <= 15 && d * L <= 128, "pccx_prob_forward_tiled: unsupported d=%d L=%d", d, L);
    PCCX_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "pccx_prob_forward_tiled: workspace must be 16-byte aligned");
    float *feature = workspace + (size_t)B * prob_feature_workgroups(S) * 256;   // a multiple of 256 floats past a 16-byte-aligned base
    const int rc = prob_feature_launch(centres, B, S, prob_blob, workspace, feature, (hipStream_t)stream);
    if (rc != PCCX_OK) return rc;
    hipLaunchKernelGGL(prob_rows_kernel<false>, dim3(((S >> 4) + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, centres, S, d, L,
                       prob_blob, feature, (const int32_t *)nullptr, 0, 0, pmf, cdf, cdf_int);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}
