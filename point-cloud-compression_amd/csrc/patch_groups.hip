// patch_groups.hip -- which patches of a batch are copies of an earlier patch of the same cloud, and the copy-back of their results.
//
// In octree_mode "reference" the patch centres come from the bug-compatible octree decode (octree.hip, octree_np.py:47-112): one byte of
// the stream is consumed, so a cloud has at most 8 distinct centres in {0.25, 0.75}^3 and rows np-1 .. 63 repeat the last one.  Everything
// downstream of a centre (kNN patch, in-patch neighbour table, latent rows; on the way back: decoded points) is a deterministic function
// of the patch's own inputs, so a transform needs to run once per distinct (cloud, key row) and its result is copied to the duplicates.
//
//   rep[p]   = the smallest patch of p's cloud whose key row equals p's bit for bit (rows are compared as uint32 words: -0 != +0, a NaN
//              equals itself); rep[p] == p marks a representative
//   uniq[]   = the representatives in ascending order, n_uniq of them -- all of it stays on the device; consumers are launched with a
//              grid sized from P and read *n_uniq themselves
//
// Three small launches: per cloud rep + count, one workgroup's exclusive scan of the counts, per cloud ordered compaction.
#include "common.h"

#define PG_MAX_S 1024

struct PgKeys {
    const unsigned *a, *b;      // (P, fa) and (P, fb) rows, b may be null
    int fa, fb;
};

__device__ __forceinline__ bool pg_rows_equal(const PgKeys &k, size_t p, size_t r)
{
    for (int c = 0; c < k.fa; ++c)
        if (k.a[p * k.fa + c] != k.a[r * k.fa + c]) return false;
    for (int c = 0; c < k.fb; ++c)
        if (k.b[p * k.fb + c] != k.b[r * k.fb + c]) return false;
    return true;
}

__global__ __launch_bounds__(256) void patch_groups_rep_kernel(PgKeys k, int S, int *__restrict__ rep, int *__restrict__ cnt)
{
    __shared__ unsigned sh[PG_MAX_S];
    __shared__ int s_cnt;
    const int tid = threadIdx.x, b = blockIdx.x;
    const size_t base = (size_t)b * S;
    if (tid == 0) s_cnt = 0;
    for (int i = tid; i < S; i += blockDim.x) {
        unsigned h = 2166136261u;                                   // a filter only: equality is decided on the rows themselves
        for (int c = 0; c < k.fa; ++c) h = (h ^ k.a[(base + i) * k.fa + c]) * 16777619u;
        for (int c = 0; c < k.fb; ++c) h = (h ^ k.b[(base + i) * k.fb + c]) * 16777619u;
        sh[i] = h;
    }
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < S; i += blockDim.x) {
        const unsigned h = sh[i];
        int r = i;
        for (int j = 0; j < i; ++j)
            if (sh[j] == h && pg_rows_equal(k, base + i, base + j)) {
                r = j;                                              // the first equal row has no earlier equal row: it is a representative
                break;
            }
        rep[base + i] = (int)(base + r);
        mine += r == i ? 1 : 0;
    }
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (tid == 0) cnt[b] = s_cnt;
}

// one workgroup: off[b] = cnt[0] + ... + cnt[b-1], *n_uniq = the total
__global__ __launch_bounds__(1024) void patch_groups_scan_kernel(const int *__restrict__ cnt, int B, int *__restrict__ off, int *__restrict__ n_uniq)
{
    __shared__ int s[1024];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < B; b0 += 1024) {
        const int v = b0 + tid < B ? cnt[b0 + tid] : 0;
        s[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int add = tid >= o ? s[tid - o] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        if (b0 + tid < B) off[b0 + tid] = carry + s[tid] - v;
        carry += s[1023];
        __syncthreads();
    }
    if (tid == 0) *n_uniq = carry;
}

__global__ __launch_bounds__(256) void patch_groups_compact_kernel(const int *__restrict__ rep, int S, const int *__restrict__ off, int *__restrict__ uniq)
{
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.x;
    const int nw = blockDim.x >> 6;
    const size_t base = (size_t)b * S;
    int at = off[b];
    for (int i0 = 0; i0 < S; i0 += blockDim.x) {
        const int i = i0 + tid;
        const bool is_rep = i < S && rep[base + i] == (int)(base + i);
        const unsigned long long bal = __ballot(is_rep);
        if (lane == 0) s_w[w] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
        for (int q = 0; q < nw; ++q) {
            before += q < w ? s_w[q] : 0;
            all += s_w[q];
        }
        if (is_rep) uniq[at + before + pccx_ballot_rank(bal)] = (int)(base + i);
        at += all;
        __syncthreads();
    }
}

extern "C" size_t pccx_patch_groups_workspace_ints(int B) { return 2 * (size_t)(B > 0 ? B : 0); }

extern "C" int pccx_patch_groups(const float *keys_a, int floats_a, const float *keys_b, int floats_b, int B, int S, int32_t *rep, int32_t *uniq,
                                 int32_t *n_uniq, int32_t *workspace, void *stream)
{
    PCCX_CHECK_ARG(n_uniq, "pccx_patch_groups: null pointer");
    hipStream_t st = (hipStream_t)stream;
    PCCX_CHECK_ARG(B >= 0 && S >= 1 && S <= PG_MAX_S, "pccx_patch_groups: need B >= 0 and 1 <= S <= %d (B=%d S=%d)", PG_MAX_S, B, S);
    PCCX_CHECK_ARG((size_t)B * (size_t)S <= 0x7FFFFFFFull, "pccx_patch_groups: B * S does not fit an int32 patch index");
    if (B == 0) {
        PCCX_CHECK_HIP(pccx_zero_async(n_uniq, 4, st));
        return PCCX_OK;
    }
    PCCX_CHECK_ARG(keys_a && rep && uniq && workspace, "pccx_patch_groups: null pointer");
    PCCX_CHECK_ARG(floats_a >= 1 && floats_b >= 0 && (floats_b == 0 || keys_b), "pccx_patch_groups: bad key widths %d, %d", floats_a, floats_b);
    const PgKeys k{(const unsigned *)keys_a, floats_b ? (const unsigned *)keys_b : nullptr, floats_a, floats_b};
    int *cnt = workspace, *off = workspace + B;
    const int threads = S <= 64 ? 64 : S <= 128 ? 128 : 256;
    hipLaunchKernelGGL(patch_groups_rep_kernel, dim3(B), dim3(threads), 0, st, k, S, rep, cnt);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(patch_groups_scan_kernel, dim3(1), dim3(1024), 0, st, (const int *)cnt, B, off, n_uniq);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(patch_groups_compact_kernel, dim3(B), dim3(threads), 0, st, (const int *)rep, S, (const int *)off, uniq);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

// pccx_patch_groups_wide: up to 8192 patches per cloud.  The all-earlier-rows compare of patch_groups_rep_kernel is O(S^2 / threads) --
// about 130 000 dependent LDS reads per thread of a 256-thread workgroup at S = 8192 with nearly every centre distinct (octree_mode
// "full"), milliseconds per cloud -- so the wide form keeps an open-addressing table in LDS instead: 16384 slots, each holding the
// LOWEST row index of the key class that owns it (-1 = empty).  A row probes linearly from its hash: an empty slot is claimed by
// compare-and-swap, a slot whose row equals it bit for bit takes the row's index by atomic min, anything else moves on.  Slots are
// never emptied and a class's rows all walk the same probe sequence, so a class owns exactly one slot and after the barrier that
// slot holds its first row: rep.  Equality is decided on the rows themselves, as in the narrow form; the hash only picks the start.
#define PG_WIDE_MAX_S 8192
#define PG_WIDE_SLOTS 16384

__global__ __launch_bounds__(1024) void patch_groups_rep_wide_kernel(PgKeys k, int S, int *__restrict__ rep, int *__restrict__ cnt)
{
    __shared__ int table[PG_WIDE_SLOTS];
    __shared__ int s_cnt;
    const int tid = threadIdx.x, b = blockIdx.x;
    const size_t base = (size_t)b * S;
    for (int i = tid; i < PG_WIDE_SLOTS; i += 1024) table[i] = -1;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int slot_of[PG_WIDE_MAX_S / 1024];
#pragma unroll
    for (int e = 0; e < PG_WIDE_MAX_S / 1024; ++e) {
        const int i = tid + 1024 * e;
        slot_of[e] = -1;
        if (i < S) {
            unsigned h = 2166136261u;
            for (int c = 0; c < k.fa; ++c) h = (h ^ k.a[(base + i) * k.fa + c]) * 16777619u;
            for (int c = 0; c < k.fb; ++c) h = (h ^ k.b[(base + i) * k.fb + c]) * 16777619u;
            int slot = (int)((h ^ (h >> 15)) & (PG_WIDE_SLOTS - 1));
            for (int probes = 0; probes < PG_WIDE_SLOTS; ++probes) {               // at most S <= 8192 slots are ever taken: an empty one is met
                int cur = ((volatile int *)table)[slot];
                if (cur < 0) cur = atomicCAS(&table[slot], -1, i);
                if (cur < 0) { slot_of[e] = slot; break; }                         // claimed: this row opens its class
                if (pg_rows_equal(k, base + i, base + cur)) {
                    atomicMin(&table[slot], i);
                    slot_of[e] = slot;
                    break;
                }
                slot = (slot + 1) & (PG_WIDE_SLOTS - 1);
            }
        }
    }
    __syncthreads();
    int mine = 0;
#pragma unroll
    for (int e = 0; e < PG_WIDE_MAX_S / 1024; ++e) {
        const int i = tid + 1024 * e;
        if (i < S) {
            const int r = slot_of[e] >= 0 ? table[slot_of[e]] : i;
            rep[base + i] = (int)(base + r);
            mine += r == i ? 1 : 0;
        }
    }
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (tid == 0) cnt[b] = s_cnt;
}

extern "C" int pccx_patch_groups_wide(const float *keys_a, int floats_a, const float *keys_b, int floats_b, int B, int S, int32_t *rep,
                                      int32_t *uniq, int32_t *n_uniq, int32_t *workspace, void *stream)
{
    PCCX_CHECK_ARG(n_uniq, "pccx_patch_groups_wide: null pointer");
    hipStream_t st = (hipStream_t)stream;
    PCCX_CHECK_ARG(B >= 0 && S >= 1 && S <= PG_WIDE_MAX_S, "pccx_patch_groups_wide: need B >= 0 and 1 <= S <= %d (B=%d S=%d)", PG_WIDE_MAX_S, B, S);
    PCCX_CHECK_ARG((size_t)B * (size_t)S <= 0x7FFFFFFFull, "pccx_patch_groups_wide: B * S does not fit an int32 patch index");
    if (B == 0) {
        PCCX_CHECK_HIP(pccx_zero_async(n_uniq, 4, st));
        return PCCX_OK;
    }
    PCCX_CHECK_ARG(keys_a && rep && uniq && workspace, "pccx_patch_groups_wide: null pointer");
    PCCX_CHECK_ARG(floats_a >= 1 && floats_b >= 0 && (floats_b == 0 || keys_b), "pccx_patch_groups_wide: bad key widths %d, %d", floats_a, floats_b);
    const PgKeys k{(const unsigned *)keys_a, floats_b ? (const unsigned *)keys_b : nullptr, floats_a, floats_b};
    int *cnt = workspace, *off = workspace + B;
    hipLaunchKernelGGL(patch_groups_rep_wide_kernel, dim3(B), dim3(1024), 0, st, k, S, rep, cnt);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(patch_groups_scan_kernel, dim3(1), dim3(1024), 0, st, (const int *)cnt, B, off, n_uniq);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(patch_groups_compact_kernel, dim3(B), dim3(256), 0, st, (const int *)rep, S, (const int *)off, uniq);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

// rows p with rep[p] != p of up to three (P, row_floats) arrays are overwritten with row rep[p] of the same array.  Representatives'
// rows are only read, so the copy is in place.  T = uint4 when rows are whole 16-byte units, else float.
template <typename T>
__global__ __launch_bounds__(256) void replicate_rows_kernel(const int *__restrict__ rep, size_t items, int W, T *a0, T *a1, T *a2)
{
    for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
        const size_t p = it / (unsigned)W;
        const int c = (int)(it - p * (unsigned)W);
        const int r = rep[p];
        if ((size_t)r == p) continue;
        const size_t src = (size_t)r * W + c;
        a0[it] = a0[src];
        if (a1) a1[it] = a1[src];
        if (a2) a2[it] = a2[src];
    }
}

extern "C" int pccx_replicate_rows(const int32_t *rep, int64_t P, int row_floats, float *a0, float *a1, float *a2, void *stream)
{
    if (P == 0) return PCCX_OK;
    PCCX_CHECK_ARG(rep && a0, "pccx_replicate_rows: null pointer");
    PCCX_CHECK_ARG(P >= 0 && P <= 0x7FFFFFFFll && row_floats >= 1, "pccx_replicate_rows: bad shape P=%lld row_floats=%d", (long long)P, row_floats);
    const bool vec = row_floats % 4 == 0 && (((uintptr_t)a0 | (uintptr_t)a1 | (uintptr_t)a2) & 15) == 0;
    const int W = vec ? row_floats / 4 : row_floats;
    const size_t items = (size_t)P * W;
    size_t blocks = (items + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;
    if (vec)
        hipLaunchKernelGGL(replicate_rows_kernel<uint4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rep, items, W, (uint4 *)a0, (uint4 *)a1, (uint4 *)a2);
    else
        hipLaunchKernelGGL(replicate_rows_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rep, items, W, a0, a1, a2);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}
