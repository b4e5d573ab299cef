// region.hip -- which patches of a whole-room cloud a box needs (region decode).
//
// One workgroup of 1024 threads, S <= 8192 decoded patch centres of ONE cloud.  Patch p is selected iff its centre, denormalised by
// pccx_denorm1 (the arithmetic of denormalize_kernel, so the float is the one ops.denormalize gives), lies in the closed box
// [lo - halo, hi + halo] on all three axes, in fp32.  A segment (G consecutive patches, one independent stream of the split .p.bin)
// is touched iff it holds a selected patch.  Out come, all ascending:
//   patch_idx  the selected patches
//   seg_idx    the touched segments
//   rows       per selected patch its row among the touched segments' patches: (rank of its segment) * G + p % G -- where the
//              probability rows, the decoded latents and the gathered centres of that patch sit in the compact arrays
//   counts     {n_sel, n_seg}
// Order comes from a ballot + block prefix scan per chunk of 1024 (the pattern of octree.hip's block_scan_flag), never from atomics:
// the lists are the same on every run.
#include "common.h"

#define REGION_MAX_S 8192

__device__ __forceinline__ int region_scan_flag(bool flag, int *s_w, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    const int incl = pccx_ballot_rank(mask) + (flag ? 1 : 0);
    if (lane == 0) s_w[w] = __popcll(mask);
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < 16; ++k) {
        const int v = s_w[k];
        if (k < w) base += v;
        tot += v;
    }
    __syncthreads();
    *total = tot;
    return incl + base;
}

__global__ __launch_bounds__(1024) void region_select_kernel(const float *__restrict__ centres, int S, const float *__restrict__ c4,
                                                             float one_minus_margin, float lx, float ly, float lz, float hx, float hy,
                                                             float hz, int G, int64_t *__restrict__ patch_idx,
                                                             int32_t *__restrict__ seg_idx, int64_t *__restrict__ rows,
                                                             int32_t *__restrict__ counts)
{
    __shared__ int s_seg[REGION_MAX_S];      // touched flag of a segment, then its rank among the touched ones
    __shared__ int s_w[16];
    const int tid = threadIdx.x;
    const int P = (S + G - 1) / G, nchunk = (S + 1023) >> 10;
    const float cx = c4[0], cy = c4[1], cz = c4[2], lg = c4[3];
    for (int s = tid; s < P; s += 1024) s_seg[s] = 0;
    __syncthreads();
    unsigned sel = 0;                        // bit c: patch c * 1024 + tid is selected
    for (int c = 0; c < nchunk; ++c) {
        const int p = (c << 10) + tid;
        if (p < S) {
            const float x = pccx_denorm1(centres[3 * p], lg, one_minus_margin, cx);
            const float y = pccx_denorm1(centres[3 * p + 1], lg, one_minus_margin, cy);
            const float z = pccx_denorm1(centres[3 * p + 2], lg, one_minus_margin, cz);
            if (lx <= x && x <= hx && ly <= y && y <= hy && lz <= z && z <= hz) {
                sel |= 1u << c;
                s_seg[p / G] = 1;            // every writer stores the same value
            }
        }
    }
    __syncthreads();
    int n_seg = 0;
    for (int s0 = 0; s0 < P; s0 += 1024) {
        const int s = s0 + tid;
        const bool f = s < P && s_seg[s] != 0;
        int tot;
        const int rank = region_scan_flag(f, s_w, &tot) - 1;
        if (f) {
            seg_idx[n_seg + rank] = s;
            s_seg[s] = n_seg + rank;
        }
        n_seg += tot;
    }
    __syncthreads();
    int n_sel = 0;
    for (int c = 0; c < nchunk; ++c) {
        const int p = (c << 10) + tid;
        const bool f = (sel >> c) & 1u;
        int tot;
        const int rank = region_scan_flag(f, s_w, &tot) - 1;
        if (f) {
            patch_idx[n_sel + rank] = p;
            rows[n_sel + rank] = (int64_t)s_seg[p / G] * G + p % G;
        }
        n_sel += tot;
    }
    if (tid == 0) {
        counts[0] = n_sel;
        counts[1] = n_seg;
    }
}

extern "C" int pccx_region_select(const float *centres, int S, const float *c4, double margin, const float *box_host, float halo, int G,
                                  int64_t *patch_idx, int32_t *seg_idx, int64_t *rows, int32_t *counts, void *stream)
{
    PCCX_CHECK_ARG(centres && c4 && box_host && patch_idx && seg_idx && rows && counts, "pccx_region_select: null pointer");
    PCCX_CHECK_ARG(S >= 1 && S <= REGION_MAX_S && G >= 1, "pccx_region_select: bad shape S=%d G=%d (1 <= S <= %d, G >= 1)", S, G, REGION_MAX_S);
    PCCX_CHECK_ARG(halo >= 0.f && halo <= 3.0e38f, "pccx_region_select: halo must be finite and not negative");
    for (int a = 0; a < 3; ++a)
        PCCX_CHECK_ARG(box_host[a] <= box_host[3 + a] && box_host[a] >= -3.0e38f && box_host[3 + a] <= 3.0e38f,
                       "pccx_region_select: box must be six finite floats with lo <= hi");
    // lo - halo and hi + halo, each rounded once in fp32 as the definition states them
    const float lx = box_host[0] - halo, ly = box_host[1] - halo, lz = box_host[2] - halo;
    const float hx = box_host[3] + halo, hy = box_host[4] + halo, hz = box_host[5] + halo;
    hipLaunchKernelGGL(region_select_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, centres, S, c4, (float)(1.0 - margin), lx, ly,
                       lz, hx, hy, hz, G, patch_idx, seg_idx, rows, counts);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}
