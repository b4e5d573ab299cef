// Nearest-n training crops cut on the GPU: pccx_crop_nearest.
//
// The store is every training cloud concatenated, (M_total, 3) f32, with an (F + 1) int64 offset table.  Slot b names a cloud, a seed
// point inside it and a count n; its crop is the n points with the smallest keys (__float_as_uint(pccx_sqdist(seed, p_i)), i), written
// in ascending i.  pccx_sqdist is never negative, so its bit pattern orders as the float does; a NaN coordinate gives the largest keys.
//
// Form: a radix select over the 32 key bits of the distance (11 / 11 / 10 from the top), then an ordered compaction.
//   crop_init_kernel      (B)      clamps the tables into a slot record and clears the slot's three histograms
//   crop_hist_kernel<0>   (G, B)   LDS histogram of bits 31..21 of its chunk, folded into the global one: one integer add per bin per workgroup
//   crop_hist_kernel<1>   (G, B)   every workgroup first resolves pass 0 (which bin the n-th key falls in), then bits 20..10 of the keys in that bin
//   crop_hist_kernel<2>   (G, B)   likewise bits 9..0
//   crop_count_kernel     (G, B)   resolves pass 2: threshold T and r = how many keys equal to T are taken; per chunk #(d < T), #(d == T)
//   crop_scan_kernel      (B)      exclusive scan of both counts over the chunks
//   crop_compact_kernel   (G, B)   point i goes to row #(d < T before i) + min(#(d == T before i), r); rows behind n: NaN / -1
// G = ceil(M_max / 4096): every grid is a function of (B, M_max) alone.  Integer atomics only, so no result depends on arrival order;
// no memset / memcpy: every table is cleared or fully written by a kernel of the call before it is read.
#include "common.h"

#define CROP_THREADS 256
#define CROP_PER_THREAD 16
#define CROP_CHUNK (CROP_THREADS * CROP_PER_THREAD)     // points per workgroup
#define CROP_BINS 2048
#define CROP_MAX_M (1 << 24)
#define CROP_MAX_NCAP 131072
#define CROP_MAX_B 1024

struct CropSlot {                  // 64 bytes per slot, written by crop_init_kernel
    long long base;                // first row of the cloud in the store
    int M, n;                      // clamped: 0 <= M <= min(M_max, rows left), 1 <= n <= min(N_cap, M) (0 for an empty cloud)
    float sx, sy, sz;
    unsigned prefix[3], k[3];      // after pass p: the key bits fixed so far, and the rank still sought among the keys that share them
    int pad_[3];
};

static inline size_t crop_chunks(long long M_max) { return (size_t)((M_max + CROP_CHUNK - 1) / CROP_CHUNK); }

// exclusive prefix of v over the 256 threads (red: 4 words of LDS); every thread also gets the total
__device__ __forceinline__ unsigned crop_block_excl(unsigned v, unsigned *red, unsigned &total)
{
    const int lane = pccx_lane(), w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        unsigned t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                   // red may still be read from the call before
    if (lane == 63) red[w] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int j = 0; j < CROP_THREADS / 64; ++j) {
        unsigned t = red[j];
        if (j < w) before += t;
        all += t;
    }
    total = all;
    return before + inc - v;
}

// Which of the NB bins of hist holds the k-th key (k counted from 1), and the rank left inside it -> res[0], res[1].  Every workgroup
// of the next pass repeats this on the same table: 8 KiB from L2 against a kernel launch.  k = 0 (an empty cloud) gives bin 0, rank 0.
template <int NB>
__device__ __forceinline__ void crop_resolve(const unsigned *__restrict__ hist, unsigned k, unsigned *red, unsigned *res)
{
    constexpr int PER = NB / CROP_THREADS;
    unsigned h[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        h[j] = hist[threadIdx.x * PER + j];
        sum += h[j];
    }
    if (threadIdx.x == 0) { res[0] = 0u; res[1] = 0u; }
    unsigned total;
    unsigned run = crop_block_excl(sum, red, total);   // its barriers order the defaults above before the write below
    if (run < k && k <= run + sum) {                   // exactly one thread
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (run < k && k <= run + h[j]) { res[0] = (unsigned)(threadIdx.x * PER + j); res[1] = k - run; }
            run += h[j];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ unsigned crop_key(const float *__restrict__ p, const CropSlot &s, int i)
{
    const float *q = p + 3 * (s.base + i);
    return __float_as_uint(pccx_sqdist(s.sx, s.sy, s.sz, q[0], q[1], q[2]));
}

__global__ __launch_bounds__(CROP_THREADS) void crop_init_kernel(const float *__restrict__ points, long long M_total,
                                                                 const int64_t *__restrict__ offsets, int F, const int32_t *__restrict__ cloud,
                                                                 const int32_t *__restrict__ seed, const int32_t *__restrict__ n, int N_cap,
                                                                 int M_max, CropSlot *__restrict__ slots, unsigned *__restrict__ hist)
{
    const int b = blockIdx.x;
    unsigned *h = hist + (size_t)b * 3 * CROP_BINS;
    for (int j = threadIdx.x; j < 3 * CROP_BINS; j += CROP_THREADS) h[j] = 0u;
    if (threadIdx.x == 0) {
        CropSlot s;
        int c = min(max(cloud[b], 0), F - 1);
        long long base = min(max((long long)offsets[c], 0ll), M_total);
        long long m = min(max((long long)offsets[c + 1] - base, 0ll), min((long long)M_max, M_total - base));
        s.base = base;
        s.M = (int)m;
        s.n = m > 0 ? min(max(n[b], 1), min(N_cap, (int)m)) : 0;
        s.sx = s.sy = s.sz = 0.f;
        if (m > 0) {
            const float *q = points + 3 * (base + min(max(seed[b], 0), (int)m - 1));
            s.sx = q[0], s.sy = q[1], s.sz = q[2];
        }
        for (int j = 0; j < 3; ++j) s.prefix[j] = 0u, s.k[j] = 0u, s.pad_[j] = 0;
        slots[b] = s;
    }
}

template <int PASS>
__global__ __launch_bounds__(CROP_THREADS) void crop_hist_kernel(const float *__restrict__ points, CropSlot *__restrict__ slots,
                                                                 unsigned *__restrict__ hist)
{
    constexpr int NB = PASS == 2 ? 1024 : CROP_BINS;
    __shared__ unsigned lh[NB];
    __shared__ unsigned red[4], res[2];
    const int b = blockIdx.y, i0 = blockIdx.x * CROP_CHUNK;
    const CropSlot s = slots[b];
    if (i0 >= s.M) return;                             // workgroup-uniform; chunk 0 of a cloud with points never leaves here
    for (int j = threadIdx.x; j < NB; j += CROP_THREADS) lh[j] = 0u;
    unsigned prefix = 0;
    if (PASS > 0) {
        const unsigned k = PASS == 1 ? (unsigned)s.n : s.k[PASS - 1];
        crop_resolve<CROP_BINS>(hist + ((size_t)b * 3 + (PASS - 1)) * CROP_BINS, k, red, res);
        prefix = PASS == 1 ? res[0] : (s.prefix[0] << 11) | res[0];
        if (blockIdx.x == 0 && threadIdx.x == 0) {     // the record of this pass is read by the kernels behind this one only
            slots[b].prefix[PASS - 1] = prefix;
            slots[b].k[PASS] = res[1];
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < CROP_PER_THREAD; ++t) {
        const int i = i0 + t * CROP_THREADS + threadIdx.x;
        if (i < s.M) {
            const unsigned d = crop_key(points, s, i);
            if (PASS == 0) atomicAdd(&lh[d >> 21], 1u);
            if (PASS == 1 && (d >> 21) == prefix) atomicAdd(&lh[(d >> 10) & 2047u], 1u);
            if (PASS == 2 && (d >> 10) == prefix) atomicAdd(&lh[d & 1023u], 1u);
        }
    }
    __syncthreads();
    unsigned *g = hist + ((size_t)b * 3 + PASS) * CROP_BINS;
    for (int j = threadIdx.x; j < NB; j += CROP_THREADS)
        if (lh[j]) atomicAdd(&g[j], lh[j]);
}

// One wave's 1024 consecutive points of the chunk: bit t of lt / eq = point i0 + wave * 1024 + t * 64 + lane is below / at the threshold
__device__ __forceinline__ void crop_classify(const float *__restrict__ points, const CropSlot &s, int i0, unsigned T, unsigned &lt, unsigned &eq)
{
    const int first = i0 + (threadIdx.x >> 6) * (64 * CROP_PER_THREAD) + pccx_lane();
    lt = eq = 0u;
#pragma unroll 4
    for (int t = 0; t < CROP_PER_THREAD; ++t) {
        const int i = first + t * 64;
        if (i < s.M) {
            const unsigned d = crop_key(points, s, i);
            lt |= (unsigned)(d < T) << t;
            eq |= (unsigned)(d == T) << t;
        }
    }
}

__global__ __launch_bounds__(CROP_THREADS) void crop_count_kernel(const float *__restrict__ points, CropSlot *__restrict__ slots,
                                                                  const unsigned *__restrict__ hist, unsigned *__restrict__ cnt, int G)
{
    __shared__ unsigned red[4], res[2];
    const int b = blockIdx.y, i0 = blockIdx.x * CROP_CHUNK;
    const CropSlot s = slots[b];
    unsigned *c = cnt + ((size_t)b * 2) * G + blockIdx.x;
    if (i0 >= s.M) {                                   // every entry of the count tables is written: the scan reads all G
        if (threadIdx.x == 0) c[0] = 0u, c[G] = 0u;
        return;
    }
    crop_resolve<1024>(hist + ((size_t)b * 3 + 2) * CROP_BINS, s.k[2], red, res);
    const unsigned T = (s.prefix[1] << 10) | res[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        slots[b].prefix[2] = T;                        // the threshold, and in k[0] how many keys equal to it the crop takes
        slots[b].k[0] = res[1];
    }
    unsigned lt, eq, total_lt, total_eq;
    crop_classify(points, s, i0, T, lt, eq);
    crop_block_excl(__popc(lt), red, total_lt);
    crop_block_excl(__popc(eq), red, total_eq);
    if (threadIdx.x == 0) c[0] = total_lt, c[G] = total_eq;
}

__global__ __launch_bounds__(CROP_THREADS) void crop_scan_kernel(unsigned *__restrict__ cnt, int G)
{
    __shared__ unsigned red[4];
    const int per = (G + CROP_THREADS - 1) / CROP_THREADS, j0 = threadIdx.x * per, j1 = min(j0 + per, G);
    for (int which = 0; which < 2; ++which) {
        unsigned *c = cnt + ((size_t)blockIdx.x * 2 + which) * G;
        unsigned sum = 0, total;
        for (int j = j0; j < j1; ++j) sum += c[j];
        unsigned run = crop_block_excl(sum, red, total);
        for (int j = j0; j < j1; ++j) {
            const unsigned v = c[j];
            c[j] = run;
            run += v;
        }
    }
}

__global__ __launch_bounds__(CROP_THREADS) void crop_compact_kernel(const float *__restrict__ points, const CropSlot *__restrict__ slots,
                                                                    const unsigned *__restrict__ cnt, int G, int N_cap,
                                                                    float *__restrict__ out, int32_t *__restrict__ out_idx)
{
    __shared__ unsigned wl[4], we[4];
    const int b = blockIdx.y, i0 = blockIdx.x * CROP_CHUNK, lane = pccx_lane(), w = threadIdx.x >> 6;
    const CropSlot s = slots[b];
    float *o = out + (size_t)b * N_cap * 3;
    int32_t *oi = out_idx ? out_idx + (size_t)b * N_cap : nullptr;
    const float nan = __uint_as_float(0x7FC00000u);
    for (int j = s.n + blockIdx.x * CROP_THREADS + threadIdx.x; j < N_cap; j += G * CROP_THREADS) {   // the rows behind the crop
        o[3 * j] = nan, o[3 * j + 1] = nan, o[3 * j + 2] = nan;
        if (oi) oi[j] = -1;
    }
    if (i0 >= s.M) return;
    const unsigned T = s.prefix[2], r = s.k[0];
    unsigned lt, eq;
    crop_classify(points, s, i0, T, lt, eq);
    unsigned nl = __popc(lt), ne = __popc(eq);
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) nl += __shfl_xor(nl, o2, 64), ne += __shfl_xor(ne, o2, 64);
    if (lane == 0) wl[w] = nl, we[w] = ne;
    __syncthreads();
    unsigned run_lt = cnt[((size_t)b * 2) * G + blockIdx.x], run_eq = cnt[((size_t)b * 2 + 1) * G + blockIdx.x];
    for (int j = 0; j < w; ++j) run_lt += wl[j], run_eq += we[j];
    const int first = i0 + w * (64 * CROP_PER_THREAD) + lane;
    for (int t = 0; t < CROP_PER_THREAD; ++t) {        // wave-uniform trip count and counters; ballots give the order inside 64 points
        const bool is_lt = (lt >> t) & 1u, is_eq = (eq >> t) & 1u;
        const unsigned long long bl = __ballot(is_lt), be = __ballot(is_eq);
        const unsigned rank_lt = run_lt + pccx_ballot_rank(bl), rank_eq = run_eq + pccx_ballot_rank(be);
        if (is_lt || (is_eq && rank_eq < r)) {
            const unsigned pos = rank_lt + min(rank_eq, r);
            if (pos < (unsigned)s.n) {                 // always true for consistent counts; keeps a store inside the slot whatever happens
                const int i = first + t * 64;
                const float *q = points + 3 * (s.base + i);
                o[3 * pos] = q[0], o[3 * pos + 1] = q[1], o[3 * pos + 2] = q[2];
                if (oi) oi[pos] = i;
            }
        }
        run_lt += (unsigned)__popcll(bl), run_eq += (unsigned)__popcll(be);
    }
}

extern "C" size_t pccx_crop_nearest_workspace_bytes(int B, int M_max)
{
    if (B < 0 || M_max < 0) return 0;
    return (size_t)B * (sizeof(CropSlot) + 3 * CROP_BINS * sizeof(unsigned) + 2 * crop_chunks(M_max) * sizeof(unsigned));
}

extern "C" int pccx_crop_nearest(const float *points, int64_t M_total, const int64_t *offsets, int F, const int32_t *cloud,
                                 const int32_t *seed, const int32_t *n, int B, int N_cap, int M_max, float *out, int32_t *out_idx,
                                 void *workspace, void *stream)
{
    PCCX_CHECK_ARG(B >= 0 && B <= CROP_MAX_B, "pccx_crop_nearest: B=%d slots, at most CROP_MAX_B = %d per call", B, CROP_MAX_B);
    PCCX_CHECK_ARG(N_cap >= 1 && N_cap <= CROP_MAX_NCAP, "pccx_crop_nearest: N_cap=%d, a crop holds 1..CROP_MAX_NCAP = %d points", N_cap,
                   CROP_MAX_NCAP);
    PCCX_CHECK_ARG(M_max >= 1 && M_max <= CROP_MAX_M, "pccx_crop_nearest: M_max=%d, a cloud holds 1..CROP_MAX_M = %d points", M_max,
                   CROP_MAX_M);
    PCCX_CHECK_ARG(F >= 1 && M_total >= 1, "pccx_crop_nearest: bad store F=%d M_total=%lld", F, (long long)M_total);
    if (B == 0) return PCCX_OK;
    PCCX_CHECK_ARG(points && offsets && cloud && seed && n && out && workspace, "pccx_crop_nearest: null pointer");
    static_assert(sizeof(CropSlot) == 64, "CropSlot is 64 bytes");
    hipStream_t st = (hipStream_t)stream;
    const int G = (int)crop_chunks(M_max);
    CropSlot *slots = (CropSlot *)workspace;
    unsigned *hist = (unsigned *)(slots + B), *cnt = hist + (size_t)B * 3 * CROP_BINS;
    const dim3 grid(G, B), block(CROP_THREADS);
    hipLaunchKernelGGL(crop_init_kernel, dim3(B), block, 0, st, points, (long long)M_total, offsets, F, cloud, seed, n, N_cap, M_max, slots, hist);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(crop_hist_kernel<0>, grid, block, 0, st, points, slots, hist);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(crop_hist_kernel<1>, grid, block, 0, st, points, slots, hist);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(crop_hist_kernel<2>, grid, block, 0, st, points, slots, hist);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(crop_count_kernel, grid, block, 0, st, points, slots, (const unsigned *)hist, cnt, G);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(crop_scan_kernel, dim3(B), block, 0, st, cnt, G);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(crop_compact_kernel, grid, block, 0, st, points, (const CropSlot *)slots, (const unsigned *)cnt, G, N_cap, out, out_idx);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}
