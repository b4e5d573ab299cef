// grid_nn.hip -- exact nearest-neighbour and K-nearest search through a uniform grid index, for clouds too large for the all-pairs
// kernels of knn.hip (whole rooms of 10^5 .. 10^6 points: pccx/large.py evaluate_large).  The results are bit for bit what
// pccx_nn_dist and pccx_knn return; the reference runs the same searches through open3d's KD-tree (eval.py:55-81) and
// pytorch3d.ops.knn_points (eval.py:132).
//
// Index (pccx_grid_index_build), one per batch (B, N, 3) of reference clouds, everything on the device:
//   1. bounding box per cloud (ordered-int atomics, as pccx_morton_keys_auto)
//   2. cubic cells, (Gx, Gy, Gz) per cloud from pccx_grid_dims -- the same function on the host and on the device
//   3. key = cloud * S + cell per point (S = the cell budget of N points + 1), the library's stable radix sort over the keys,
//      the points copied in that order (coordinates and original index) and a cell-start table by binary search in the sorted keys
// Query (pccx_grid_nn / pccx_grid_knn): the queries' own cell keys are sorted with the same sort and ONE WAVE takes one query, in
// that order, so neighbouring waves read the same cells from cache.  The wave walks the query's cell, then the shell of cells at
// Chebyshev distance 1, 2, ... around it; the 64 lanes read 64 consecutive points of a run of cells (coalesced: the points lie in
// cell order) and the best K (distance, index) pairs live one per lane in registers (K <= 32; no LDS, no scratch).
// Query with a wide K (pccx_grid_knn_wide, K <= 1024: the codec's patches): one WORKGROUP per query and the candidates in LDS -- the
// comment above grid_wide_kernel at the end of this file.
//
// Why the results are exact:
//   * Same arithmetic.  Every distance is pccx_sqdist(query, point), the operation sequence of nn_dist_kernel and knn_kernel, and
//     this file is built with -ffp-contract=off like knn.hip: a pair has the same fp32 distance in both searches.
//   * Same tie rule.  Candidates are compared as (distance bits, index) pairs, so among equal distances the lower index wins whatever
//     the visiting order (nn_dist_kernel's first minimum, pccx_knn's composite key).  Hence the walk may only stop when the K-th best
//     distance is STRICTLY below the bound: an unvisited point at exactly that distance could carry a lower index.
//   * Conservative bound.  After ring r the cells [c - r, c + r] of every axis are visited.  An unvisited point lies beyond a face of
//     that cube which still has cells behind it, so its distance is at least the query's distance to the nearest such face.  Cells
//     come from floorf((v - lo) * inv) in fp32, the faces from c * cell in fp32; the two can disagree by a few ulp of
//     max(extent, |query - lo|), so every gap is shrunk by GRID_SLACK of that magnitude (30 ulp; the roundings add up to about 5)
//     and the squared bound by 1e-4 against the roundings of the distance itself -- as bq_grid_build_kernel takes 1.0001 on its cell.
//     A query outside the box is clamped to a border cell for the walk but the gaps use its true coordinates: towards the box they
//     are <= 0 until the cube reaches the query's side, which keeps the walk going.
// The ring loop is an integer loop bounded by max(Gx, Gy, Gz) <= GRID_MAX_AXIS; every float comparison can only END it early.
// Cost of the worst case: a query far outside the box (or one whose coordinates are NaN) never meets its bound before the cube covers
// the grid, so its ONE wave visits every cell -- up to GRID_MAX_CELLS of them, column by column, two dependent cell-start loads per
// column.  Bounded and exact, but up to seconds for such a query on a 2^21-cell grid; reconstructions stay within a few cells of the box.
#include <float.h>
#include <math.h>

#include "common.h"

// The two constants that shape the grid.  Both are first choices, not yet fixed from a measurement: DESIGN 4.5 says what is known of
// them and names the command that produces the table (tools/experiments/grid_nn_cost.py).  pccx.h and tests/test_grid_nn_cpu.py state
// the same two values.
#define GRID_TARGET 2                      // points per cell of the box's volume (or area / length for flat boxes) aimed at
#define GRID_MAX_CELLS (1 << 21)           // cells per cloud at most: 8 MiB of cell starts; binds above 4 * 2^20 points only
#define GRID_MAX_AXIS 1024                 // cells per axis at most: bounds the ring loop
#define GRID_KMAX 32
#define GRID_SLACK 2e-6f
#define GRID_PARAM_WORDS 16                // per cloud: [0..5] bbox (ordered ints), [6] cell, [7] 1/cell, [8..10] Gx Gy Gz

// ------------------------------------------------------------------------------------------
// grid dimensions: a pure function of (N, extents), shared by the host (pccx_grid_dims, the workspace size) and the device
// ------------------------------------------------------------------------------------------
__host__ __device__ static inline long long grid_cell_budget(long long N)
{
    long long c = N / GRID_TARGET;
    c = c > GRID_MAX_CELLS ? GRID_MAX_CELLS : c;
    return c < 1 ? 1 : c;
}

__host__ __device__ static inline float grid_clean_extent(float e) { return (e > 1e-30f && e < FLT_MAX) ? e : 0.f; }   // NaN, inf, <= 0: no extent

// cells along an axis of extent e when the longest axis (emax) has g cells: the cell index of its far end + 1, at most g
__host__ __device__ static inline int grid_axis_cells(float e, float emax, int g)
{
    const float cell = emax / (float)g;
    const float f = fminf(floorf(e / cell), (float)(g - 1));
    return (f >= 0.f ? (int)f : 0) + 1;
}

// Largest g <= GRID_MAX_AXIS whose grid has at most the budget's cells.  Division and floor are correctly rounded and monotone, so
// every axis count is non-decreasing in g and the search is well defined; an axis of zero extent gets one cell, a cloud of identical
// points one cell in all (cell side 1: never used to separate anything).  budget: the cells a cloud may have, >= 1.
__host__ __device__ static inline void grid_dims_budget(long long budget, float ex, float ey, float ez, int *G, float *cell)
{
    const float e[3] = {grid_clean_extent(ex), grid_clean_extent(ey), grid_clean_extent(ez)};
    const float emax = fmaxf(fmaxf(e[0], e[1]), e[2]);
    G[0] = G[1] = G[2] = 1;
    *cell = 1.f;
    if (!(emax > 0.f)) return;
    int lo = 1, hi = GRID_MAX_AXIS;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const long long cells = (long long)grid_axis_cells(e[0], emax, mid) * grid_axis_cells(e[1], emax, mid) * grid_axis_cells(e[2], emax, mid);
        if (cells <= budget) lo = mid;
        else hi = mid - 1;
    }
    for (int a = 0; a < 3; ++a) G[a] = grid_axis_cells(e[a], emax, lo);
    *cell = emax / (float)lo;
}

__host__ __device__ static inline void grid_dims(long long N, float ex, float ey, float ez, int *G, float *cell)
{
    grid_dims_budget(grid_cell_budget(N), ex, ey, ez, G, cell);
}

extern "C" int pccx_grid_dims(int N, float ex, float ey, float ez, int32_t *dims, float *cell)
{
    PCCX_CHECK_ARG(dims && cell && N >= 1, "pccx_grid_dims: bad arguments (N=%d)", N);
    int G[3];
    grid_dims(N, ex, ey, ez, G, cell);
    dims[0] = G[0]; dims[1] = G[1]; dims[2] = G[2];
    return PCCX_OK;
}

// ------------------------------------------------------------------------------------------
// workspace layout (every part 16-byte aligned)
// ------------------------------------------------------------------------------------------
struct GridLayout {
    size_t params, cstart, sxyz, sidx, keys, order, sort, total;
    long long S;                                     // key stride of a cloud: its cell budget + 1
};

static inline size_t grid_align(size_t v) { return (v + 15) / 16 * 16; }

extern "C" size_t pccx_sort_keys_workspace_bytes(int64_t n);
extern "C" int pccx_sort_keys_u64(int64_t *keys, int64_t n, int key_bits, int64_t *order, void *workspace, void *stream);

static GridLayout grid_layout(int B, int N)
{
    GridLayout L;
    const size_t n = (size_t)B * (size_t)N;
    L.S = grid_cell_budget(N) + 1;
    size_t o = 0;
    L.params = o; o += grid_align((size_t)B * GRID_PARAM_WORDS * 4);
    L.cstart = o; o += grid_align(((size_t)B * (size_t)L.S + 1) * 4);
    L.sxyz = o; o += grid_align(n * 12);
    L.sidx = o; o += grid_align(n * 4);
    L.keys = o; o += grid_align(n * 8);
    L.order = o; o += grid_align(n * 8);
    L.sort = o; o += grid_align(pccx_sort_keys_workspace_bytes((int64_t)n));
    L.total = o;
    return L;
}

extern "C" size_t pccx_grid_index_workspace_bytes(int B, int N)
{
    if (B <= 0 || N <= 0) return 0;
    return grid_layout(B, N).total;
}

// scratch of one query call over (B, M) queries: their cell keys, the sorted order and the sort's own workspace
extern "C" size_t pccx_grid_query_workspace_bytes(int B, int M)
{
    if (B <= 0 || M <= 0) return 0;
    const size_t n = (size_t)B * (size_t)M;
    return 2 * grid_align(n * 8) + grid_align(pccx_sort_keys_workspace_bytes((int64_t)n));
}

static inline int grid_key_bits(int B, long long S)
{
    unsigned long long top = (unsigned long long)B * (unsigned long long)S;      // keys are < B * S
    int bits = 1;
    while (bits < 64 && (top >> bits) != 0ull) ++bits;
    return bits;
}

// ------------------------------------------------------------------------------------------
// build kernels
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int grid_ordered_int(float f)
{
    const int b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float grid_ordered_float(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__global__ void grid_bbox_init_kernel(int *__restrict__ params, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * GRID_PARAM_WORDS) return;
    const int w = i % GRID_PARAM_WORDS;
    params[i] = w < 3 ? 0x7fffffff : (w < 6 ? (int)0x80000000 : 0);
}

__global__ __launch_bounds__(256) void grid_bbox_kernel(const float *__restrict__ xyz, int N, int *__restrict__ params)
{
    const int b = blockIdx.y;
    const float *p = xyz + (size_t)b * N * 3;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = p[3 * (size_t)i + a];
            lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v);
        }
    __shared__ float red[4][6];                       // one atomic per component per workgroup (geometry.hip: bbox_kernel)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
        if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][a] = lo[a]; red[threadIdx.x >> 6][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        atomicMin(params + b * GRID_PARAM_WORDS + a, grid_ordered_int(fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]))));
        atomicMax(params + b * GRID_PARAM_WORDS + 3 + a,
                  grid_ordered_int(fmaxf(fmaxf(red[0][3 + a], red[1][3 + a]), fmaxf(red[2][3 + a], red[3][3 + a]))));
    }
}

__global__ void grid_params_kernel(int *__restrict__ params, int B, long long budget)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int *w = params + b * GRID_PARAM_WORDS;
    float e[3];
    for (int a = 0; a < 3; ++a) e[a] = __fsub_rn(grid_ordered_float(w[3 + a]), grid_ordered_float(w[a]));
    int G[3];
    float cell;
    grid_dims_budget(budget, e[0], e[1], e[2], G, &cell);
    w[6] = __float_as_int(cell);
    w[7] = __float_as_int(__fdiv_rn(1.f, cell));
    w[8] = G[0]; w[9] = G[1]; w[10] = G[2];
}

// what a cloud's queries and points need of its parameters
struct GridParams {
    float lo[3], cell, inv;
    int G[3];
};

__device__ __forceinline__ GridParams grid_load_params(const int *__restrict__ params, int b)
{
    const int *w = params + b * GRID_PARAM_WORDS;
    GridParams g;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = grid_ordered_float(w[a]);
        const int G = w[8 + a];
        g.G[a] = G < 1 ? 1 : (G > GRID_MAX_AXIS ? GRID_MAX_AXIS : G);       // whatever the memory holds, the walk stays bounded
    }
    g.cell = __int_as_float(w[6]);
    g.inv = __int_as_float(w[7]);
    return g;
}

// cell of a coordinate, clamped in float first: NaN and out-of-range values land in [0, G - 1] before the conversion
__device__ __forceinline__ int grid_cell(float v, float lo, float inv, int G)
{
    const float f = floorf(__fmul_rn(__fsub_rn(v, lo), inv));
    return (int)fminf(fmaxf(f, 0.f), (float)(G - 1));
}

__device__ __forceinline__ int grid_cell_id(const GridParams &g, float x, float y, float z)
{
    return (grid_cell(x, g.lo[0], g.inv, g.G[0]) * g.G[1] + grid_cell(y, g.lo[1], g.inv, g.G[1])) * g.G[2] + grid_cell(z, g.lo[2], g.inv, g.G[2]);
}

// key of point i of cloud b = b * S + its cell in cloud b's grid (pts: (B, n, 3); the grid is the INDEX's, also for query points)
__global__ __launch_bounds__(256) void grid_keys_kernel(const float *__restrict__ pts, int n, const int *__restrict__ params, long long S,
                                                        long long *__restrict__ keys)
{
    const int b = blockIdx.y;
    const GridParams g = grid_load_params(params, b);
    const float *p = pts + (size_t)b * n * 3;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        keys[(size_t)b * n + i] = (long long)b * S + grid_cell_id(g, p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]);
}

// the points in key order: coordinates and index inside their cloud
__global__ __launch_bounds__(256) void grid_gather_kernel(const float *__restrict__ xyz, int N, long long total, const long long *__restrict__ order,
                                                          float *__restrict__ sxyz, int *__restrict__ sidx)
{
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
        const long long src = order[p];
        sxyz[3 * p] = xyz[3 * src]; sxyz[3 * p + 1] = xyz[3 * src + 1]; sxyz[3 * p + 2] = xyz[3 * src + 2];
        sidx[p] = (int)(src % N);
    }
}

// cstart[k] = first sorted position whose key is >= k, for k = 0 .. B * S (binary search: no serial fill over runs of empty cells)
__global__ __launch_bounds__(256) void grid_cell_start_kernel(const long long *__restrict__ skeys, long long total, long long entries,
                                                              int *__restrict__ cstart)
{
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < entries; k += (long long)gridDim.x * blockDim.x) {
        long long lo = 0, hi = total;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (skeys[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        cstart[k] = (int)lo;
    }
}

static inline unsigned grid_blocks(long long n, long long cap)
{
    long long b = (n + 255) / 256;
    b = b > cap ? cap : b;
    return (unsigned)(b < 1 ? 1 : b);
}

// budget: the cells per cloud, 1 <= budget <= grid_cell_budget(N) -- the layout (and its key stride S) is always that of the default
// target, so an index with coarser cells is queried exactly like any other: the grid itself is read from its parameters
static int grid_build(const char *who, const float *Y, int B, int N, long long budget, void *workspace, void *stream)
{
    PCCX_CHECK_ARG(Y && workspace && ((uintptr_t)workspace & 15) == 0, "%s: null or misaligned pointer", who);
    PCCX_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1, "%s: bad shape B=%d N=%d (1 <= B <= 65535, N >= 1)", who, B, N);
    PCCX_CHECK_ARG((long long)B * N < (1ll << 31), "%s: B * N = %lld must stay below 2^31", who, (long long)B * N);
    const GridLayout L = grid_layout(B, N);
    char *ws = (char *)workspace;
    int *params = (int *)(ws + L.params), *cstart = (int *)(ws + L.cstart), *sidx = (int *)(ws + L.sidx);
    float *sxyz = (float *)(ws + L.sxyz);
    long long *keys = (long long *)(ws + L.keys), *order = (long long *)(ws + L.order);
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)B * N;
    hipLaunchKernelGGL(grid_bbox_init_kernel, dim3((B * GRID_PARAM_WORDS + 255) / 256), dim3(256), 0, st, params, B);
    hipLaunchKernelGGL(grid_bbox_kernel, dim3(grid_blocks(N, B > 1 ? 8 : 512), B), dim3(256), 0, st, Y, N, params);
    hipLaunchKernelGGL(grid_params_kernel, dim3((B + 63) / 64), dim3(64), 0, st, params, B, budget);
    hipLaunchKernelGGL(grid_keys_kernel, dim3(grid_blocks(N, 2048), B), dim3(256), 0, st, Y, N, (const int *)params, L.S, keys);
    PCCX_CHECK_LAUNCH();
    const int rc = pccx_sort_keys_u64((int64_t *)keys, total, grid_key_bits(B, L.S), (int64_t *)order, ws + L.sort, stream);
    if (rc != PCCX_OK) return rc;
    hipLaunchKernelGGL(grid_gather_kernel, dim3(grid_blocks(total, 4096)), dim3(256), 0, st, Y, N, total, (const long long *)order, sxyz, sidx);
    const long long entries = (long long)B * L.S + 1;
    hipLaunchKernelGGL(grid_cell_start_kernel, dim3(grid_blocks(entries, 4096)), dim3(256), 0, st, (const long long *)keys, total, entries, cstart);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

extern "C" int pccx_grid_index_build(const float *Y, int B, int N, void *workspace, void *stream)
{
    return grid_build("pccx_grid_index_build", Y, B, N, grid_cell_budget(N), workspace, stream);
}

// the same index with about `target` points per cell instead of GRID_TARGET: coarser cells for searches with a wide K
extern "C" int pccx_grid_index_build_target(const float *Y, int B, int N, int target, void *workspace, void *stream)
{
    PCCX_CHECK_ARG(target >= GRID_TARGET && N >= 1, "pccx_grid_index_build_target: target=%d points per cell (at least %d: the index's layout), N=%d",
                   target, GRID_TARGET, N);
    const long long budget = N / target < 1 ? 1 : N / target, most = grid_cell_budget(N);
    return grid_build("pccx_grid_index_build_target", Y, B, N, budget < most ? budget : most, workspace, stream);
}

// ------------------------------------------------------------------------------------------
// the walk: one wave per query
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long grid_shfl64(unsigned long long v, int src)
{
    return ((unsigned long long)(unsigned)__shfl((int)(v >> 32), src) << 32) | (unsigned)__shfl((int)(unsigned)v, src);
}
__device__ __forceinline__ unsigned long long grid_shfl_up64(unsigned long long v)
{
    return ((unsigned long long)(unsigned)__shfl_up((int)(v >> 32), 1) << 32) | (unsigned)__shfl_up((int)(unsigned)v, 1);
}
__device__ __forceinline__ unsigned long long grid_wave_min64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = ((unsigned long long)(unsigned)__shfl_xor((int)(v >> 32), off) << 32) | (unsigned)__shfl_xor((int)(unsigned)v, off);
        v = o < v ? o : v;
    }
    return v;
}

// State of a wave's search.  KNN: lane k holds the k-th best (distance bits, index) key, ascending, ~0 where nothing is held yet;
// kth = the key of lane K - 1 (wave-uniform).  1-NN: every lane keeps the best key of the points IT saw; the wave minimum is taken
// once per ring.  Distances are >= +0, so the unsigned order of the bits is the order of the floats.
template <bool KNN>
__device__ __forceinline__ void grid_scan_run(const float *__restrict__ sxyz, const int *__restrict__ sidx, int p0, int p1, float qx, float qy,
                                              float qz, int K, int lane, unsigned long long &mine, unsigned long long &kth)
{
    for (int base = p0; base < p1; base += 64) {              // wave-uniform bounds
        const int p = base + lane;
        const bool valid = p < p1;
        unsigned long long key = ~0ull;
        if (valid) {
            const float d = pccx_sqdist(qx, qy, qz, sxyz[3 * (size_t)p], sxyz[3 * (size_t)p + 1], sxyz[3 * (size_t)p + 2]);
            key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)sidx[p];
            // nn_dist_kernel takes a point only on d < best with best starting at +inf: a distance of +inf or NaN is never taken
            if (!KNN && !(d < INFINITY)) key = ~0ull;
        }
        if (!KNN) {
            mine = key < mine ? key : mine;
            continue;
        }
        unsigned long long cand = __ballot(valid && key < kth);
        while (cand) {                                        // wave-uniform: one insertion per candidate still below the K-th best
            const int src = __ffsll((long long)cand) - 1;
            cand &= cand - 1;
            const unsigned long long ck = grid_shfl64(key, src);
            if (ck < kth) {
                const bool gt = mine > ck;                    // these lanes move one place up, the first of them takes the candidate
                const unsigned long long up = grid_shfl_up64(mine);
                const bool prev_gt = __shfl_up((int)gt, 1) != 0 && lane > 0;
                mine = gt ? (prev_gt ? up : ck) : mine;
                kth = grid_shfl64(mine, K - 1);
            }
        }
    }
}

// Squared lower bound on the distance from query q (cell c) to any point outside the cube of cells [c - r, c + r]: the nearest face of
// that cube that still has cells behind it, from the query's true coordinates, shrunk as the file header says.  +inf when no face has.
// The one statement of the stop rule's bound: both walks (one wave per query, one workgroup per query) end on it.
__device__ __forceinline__ float grid_face_bound2(const GridParams &g, const float (&q)[3], const int (&c)[3], int r)
{
    float bound = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float rel = __fsub_rn(q[a], g.lo[a]);
        const float slack = GRID_SLACK * (fabsf(rel) + (float)g.G[a] * g.cell);
        if (c[a] - r > 0) {
            const float gap = rel - (float)(c[a] - r) * g.cell - slack;
            bound = gap < bound ? gap : bound;
        }
        if (c[a] + r + 1 < g.G[a]) {
            const float gap = (float)(c[a] + r + 1) * g.cell - rel - slack;
            bound = gap < bound ? gap : bound;
        }
    }
    bound = bound > 0.f ? bound : 0.f;
    return bound * bound * 0.9999f;
}

template <bool KNN>
__global__ __launch_bounds__(256) void grid_walk_kernel(const float *__restrict__ X, int B, int M, int Q, const int *__restrict__ params,
                                                        const int *__restrict__ cstart, long long S, const float *__restrict__ sxyz,
                                                        const int *__restrict__ sidx, const long long *__restrict__ qorder, int K,
                                                        float *__restrict__ dists, int64_t *__restrict__ idx64, int32_t *__restrict__ idx32)
{
    const int lane = threadIdx.x & 63;
    const long long slot = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (slot >= (long long)B * M) return;                     // whole wave exits together; no block barrier below
    const long long qi = qorder[slot];                        // queries in the order of their cells
    const int b = (int)(qi / M);
    const GridParams g = grid_load_params(params, b);
    const float qx = X[3 * qi], qy = X[3 * qi + 1], qz = X[3 * qi + 2];
    const float q[3] = {qx, qy, qz};
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = grid_cell(q[a], g.lo[a], g.inv, g.G[a]);
    const int *cs = cstart + (size_t)b * S;
    const int rmax = max(max(g.G[0], g.G[1]), g.G[2]) - 1;    // ring rmax covers the grid from any cell

    unsigned long long mine = ~0ull, kth = ~0ull;
    if (!KNN) mine = kth = ((unsigned long long)0x7f800000u << 32) | 0xffffffffu;      // (+inf, -1): what nn_dist_kernel starts from
    for (int r = 0; r <= rmax; ++r) {
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.G[0] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.G[1] - 1);
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.G[2] - 1);
        for (int ix = x0; ix <= x1; ++ix)
            for (int iy = y0; iy <= y1; ++iy) {
                const int col = (ix * g.G[1] + iy) * g.G[2];
                if (abs(ix - c[0]) == r || abs(iy - c[1]) == r) {
                    // a column on the shell's side: its cells z0 .. z1 are one contiguous run of the sorted points
                    grid_scan_run<KNN>(sxyz, sidx, cs[col + z0], cs[col + z1 + 1], qx, qy, qz, K, lane, mine, kth);
                } else {                                      // inside the shell's outline (r > 0 here): its bottom and top cell only
                    if (c[2] - r >= 0) grid_scan_run<KNN>(sxyz, sidx, cs[col + c[2] - r], cs[col + c[2] - r + 1], qx, qy, qz, K, lane, mine, kth);
                    if (c[2] + r < g.G[2]) grid_scan_run<KNN>(sxyz, sidx, cs[col + c[2] + r], cs[col + c[2] + r + 1], qx, qy, qz, K, lane, mine, kth);
                }
            }
        // every cell visited?  (integers only: this is what ends the loop when no distance ever does)
        if (c[0] - r <= 0 && c[0] + r >= g.G[0] - 1 && c[1] - r <= 0 && c[1] + r >= g.G[1] - 1 && c[2] - r <= 0 && c[2] + r >= g.G[2] - 1) break;
        if (!KNN) kth = grid_wave_min64(mine);
        const float bound2 = grid_face_bound2(g, q, c, r);
        if (__uint_as_float((unsigned)(kth >> 32)) < bound2) break;       // strict: see "same tie rule" above
    }
    if (KNN) {
        if (lane < K) {
            const size_t o = (size_t)qi * K + lane;
            dists[o] = __uint_as_float((unsigned)(mine >> 32));
            idx64[o] = (int64_t)(int)(unsigned)mine;
        }
    } else {
        kth = grid_wave_min64(mine);
        if (lane == 0) {
            dists[qi] = __uint_as_float((unsigned)(kth >> 32));
            if (idx32) idx32[qi] = (int)(unsigned)kth;
        }
    }
}

static int grid_query(const char *who, bool knn, const float *X, int B, int M, int Q, const void *index, void *query_workspace, int K, float *dists,
                      int64_t *idx64, int32_t *idx32, void *stream)
{
    PCCX_CHECK_ARG(X && index && query_workspace && dists && (!knn || idx64), "%s: null pointer", who);
    PCCX_CHECK_ARG((((uintptr_t)index | (uintptr_t)query_workspace) & 15) == 0, "%s: the index and the query workspace must be 16-byte aligned", who);
    PCCX_CHECK_ARG(B >= 1 && B <= 65535 && M >= 1 && Q >= 1, "%s: bad shape B=%d queries=%d Q=%d (1 <= B <= 65535, both clouds non-empty)", who, B, M, Q);
    PCCX_CHECK_ARG((long long)B * M < (1ll << 31) && (long long)B * Q < (1ll << 31), "%s: B * points must stay below 2^31", who);
    if (knn) PCCX_CHECK_ARG(K >= 1 && K <= GRID_KMAX && K <= Q, "%s: need 1 <= K <= min(Q,%d), got K=%d Q=%d", who, GRID_KMAX, K, Q);
    const GridLayout L = grid_layout(B, Q);
    const char *ws = (const char *)index;
    const int *params = (const int *)(ws + L.params), *cstart = (const int *)(ws + L.cstart), *sidx = (const int *)(ws + L.sidx);
    const float *sxyz = (const float *)(ws + L.sxyz);
    const long long total = (long long)B * M;
    long long *qkeys = (long long *)query_workspace;
    long long *qorder = (long long *)((char *)query_workspace + grid_align((size_t)total * 8));
    void *qsort = (char *)query_workspace + 2 * grid_align((size_t)total * 8);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grid_keys_kernel, dim3(grid_blocks(M, 2048), B), dim3(256), 0, st, X, M, params, L.S, qkeys);
    PCCX_CHECK_LAUNCH();
    const int rc = pccx_sort_keys_u64((int64_t *)qkeys, total, grid_key_bits(B, L.S), (int64_t *)qorder, qsort, stream);
    if (rc != PCCX_OK) return rc;
    const unsigned blocks = (unsigned)((total + 3) / 4);
    if (knn)
        hipLaunchKernelGGL((grid_walk_kernel<true>), dim3(blocks), dim3(256), 0, st, X, B, M, Q, params, cstart, L.S, sxyz, sidx,
                           (const long long *)qorder, K, dists, idx64, (int32_t *)nullptr);
    else
        hipLaunchKernelGGL((grid_walk_kernel<false>), dim3(blocks), dim3(256), 0, st, X, B, M, Q, params, cstart, L.S, sxyz, sidx,
                           (const long long *)qorder, 1, dists, (int64_t *)nullptr, idx32);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

extern "C" int pccx_grid_nn(const float *X, int B, int P, int Q, const void *index, void *query_workspace, float *d2, int32_t *nn, void *stream)
{
    return grid_query("pccx_grid_nn", false, X, B, P, Q, index, query_workspace, 1, d2, nullptr, nn, stream);
}

extern "C" int pccx_grid_knn(const float *q, int B, int M, int N, int K, const void *index, void *query_workspace, float *dists, int64_t *idx,
                             void *stream)
{
    return grid_query("pccx_grid_knn", true, q, B, M, N, index, query_workspace, K, dists, idx, nullptr, stream);
}

// ------------------------------------------------------------------------------------------
// the wide walk: one workgroup per query, K <= 1024 (the codec's patch search, compress.py:70-74,105-108, on clouds past the 32768
// points pccx_knn keeps in LDS).  Meant for K > GRID_KMAX; smaller K are served too, for the nn and rep arguments the narrow walk lacks.
//
// The K best no longer fit one per lane, so they live in LDS: `buf` collects every scanned point whose key is below a threshold
// `thr` (~0 until K points are held), and whenever it may fill up a bitonic sort of its entries keeps the K smallest and lowers thr to
// the K-th.  Nothing below the final K-th key is ever dropped: an entry is refused or cut only when K keys below it are already held.
// The three points of the argument at the top of this file carry over unchanged: (1) distances are pccx_sqdist; (2) keys are
// (distance bits, original index) and all distinct, so the K smallest are one well-defined set whatever the visiting order; (3) after
// every ring the buffer is sorted when it holds K or more, thr IS the K-th best, and the walk ends only when its distance is
// STRICTLY below grid_face_bound2 -- or when the integer test says that every cell has been visited.
//
// All 256 threads walk the same loops (every barrier is reached by all of them):
//   ring r -> its columns in batches of 128 (two run slots each: a side column's cells z0..z1, or an inner column's bottom and top
//   cell) -> a block scan of the runs' lengths -> the batch's points 256 at a time, each thread finding its point's run by binary
//   search in the scanned offsets: every lane has a point however short the runs are.
// Appending is ballot + mbcnt per wave and one LDS atomic per wave.  `ub`, an upper bound of the count that every thread keeps in a
// register (+256 per step), says when the exact count has to be read and, if fewer than 256 places are left, the buffer compacted; a
// full buffer is thus never written to.  Every loop is bounded by integers: rings by rmax, batches by the column count, steps by the
// batch's point count, the sort by its fixed network.  One cell holding the whole cloud is one long run: N / 256 steps.
// ------------------------------------------------------------------------------------------
#define GRID_WIDE_KMAX 1024
#define GRID_WIDE_CAP 2048                 // keys of LDS per workgroup: 16 KiB, >= K + 256 for every K

extern "C" size_t pccx_grid_knn_wide_workspace_bytes(int B, int N)
{
    if (B <= 0 || N <= 0) return 0;
    return grid_align((size_t)B * (size_t)N * 4);
}

// inv[cloud * N + original index] = position in the cell-ordered copy (position p belongs to cloud p / N: the keys sort by cloud first)
__global__ __launch_bounds__(256) void grid_inverse_kernel(const int *__restrict__ sidx, int N, long long total, int *__restrict__ inv)
{
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x)
        inv[p / N * N + sidx[p]] = (int)p;
}

// Ascending bitonic sort of buf[0 .. n) (n a power of two, 2 <= n <= GRID_WIDE_CAP) by the workgroup; ends with a barrier.
__device__ __forceinline__ void grid_wide_sort(unsigned long long *buf, int n, int tid)
{
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (n >> 1); t += 256) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), l = i | stride;
                const unsigned long long a = buf[i], b = buf[l];
                if ((a > b) == ((i & size) == 0)) { buf[i] = b; buf[l] = a; }
            }
            __syncthreads();
        }
}

// Sort the c entries of buf and keep the K smallest.  Called by all threads with the same c, after a barrier behind the last append.
// Returns the count kept; thr becomes the K-th key once K are held.
__device__ __forceinline__ int grid_wide_compact(unsigned long long *buf, int *s_count, int c, int K, int tid, unsigned long long &thr)
{
    int n = 2;
    while (n < c) n <<= 1;                                    // c <= GRID_WIDE_CAP, a power of two
    for (int t = c + tid; t < n; t += 256) buf[t] = ~0ull;
    __syncthreads();
    grid_wide_sort(buf, n, tid);
    if (c >= K) thr = buf[K - 1];
    if (c > K && tid == 0) *s_count = K;
    __syncthreads();                                          // nobody appends before everybody has read thr and the count is set
    return c > K ? K : c;
}

__global__ __launch_bounds__(256) void grid_wide_kernel(const float *__restrict__ X, int B, int M, int N, const int *__restrict__ params,
                                                        const int *__restrict__ cstart, long long S, const float *__restrict__ sxyz,
                                                        const int *__restrict__ sidx, const int *__restrict__ inv, int K,
                                                        const int *__restrict__ rep, float *__restrict__ dists, int64_t *__restrict__ idx64,
                                                        float *__restrict__ nn, float patch_scale)
{
    __shared__ unsigned long long buf[GRID_WIDE_CAP];
    __shared__ int s_off[256], s_p0[256], s_wsum[4], s_count;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long qi = blockIdx.x;
    if (rep && rep[qi] != (int)qi) return;                    // a copy of an earlier query (patch_groups.hip): the whole workgroup leaves
    const int b = (int)(qi / M);
    const GridParams g = grid_load_params(params, b);
    const float q[3] = {X[3 * qi], X[3 * qi + 1], X[3 * qi + 2]};
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = grid_cell(q[a], g.lo[a], g.inv, g.G[a]);
    const int *cs = cstart + (size_t)b * S;
    const int rmax = max(max(g.G[0], g.G[1]), g.G[2]) - 1;
    const int cap = K <= 256 ? GRID_WIDE_CAP / 2 : GRID_WIDE_CAP;     // small K: compact sooner, sort less

    if (tid == 0) s_count = 0;
    __syncthreads();
    unsigned long long thr = ~0ull;
    int ub = 0;                                               // >= the count, the same in every thread
    int kept = -1;                                            // the count the last compaction left: while the count equals it, buf is sorted
    for (int r = 0; r <= rmax; ++r) {
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.G[0] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.G[1] - 1);
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.G[2] - 1);
        const int ny = y1 - y0 + 1, ncol = (x1 - x0 + 1) * ny;
        for (int n0 = 0; n0 < ncol; n0 += 128) {
            // ---- this thread's run: slot (tid & 1) of column n0 + (tid >> 1)
            const int n = n0 + (tid >> 1);
            int p0 = 0, len = 0;
            if (n < ncol) {
                const int ix = x0 + n / ny, iy = y0 + n % ny;
                const int col = (ix * g.G[1] + iy) * g.G[2];
                int za = 0, zb = -1;                          // cells za .. zb of the column; none when zb < za
                if (abs(ix - c[0]) == r || abs(iy - c[1]) == r) {
                    if ((tid & 1) == 0) { za = z0; zb = z1; } // a column on the shell's side: one contiguous run of the sorted points
                } else if ((tid & 1) == 0) {                  // inside the shell's outline (r > 0 here): its bottom and its top cell
                    if (c[2] - r >= 0) za = zb = c[2] - r;
                } else if (c[2] + r < g.G[2])
                    za = zb = c[2] + r;
                if (zb >= za) {
                    p0 = cs[col + za];
                    len = cs[col + zb + 1] - p0;
                    len = len > 0 ? len : 0;
                }
            }
            // ---- exclusive scan of the lengths over the workgroup
            int incl = len;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            __syncthreads();                                  // the previous batch's steps have read s_off / s_p0 / s_wsum
            if (lane == 63) s_wsum[w] = incl;
            __syncthreads();
            int before = 0, T = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { before += k < w ? s_wsum[k] : 0; T += s_wsum[k]; }
            s_off[tid] = before + incl - len;
            s_p0[tid] = p0;
            __syncthreads();
            // ---- the batch's T points, 256 per step
            for (int base = 0; base < T; base += 256) {
                if (ub + 256 > cap) {                         // the buffer may lack room for this step: read the count, compact if it does
                    __syncthreads();
                    const int cnt = s_count;
                    __syncthreads();
                    ub = cnt;
                    if (cnt + 256 > cap) ub = kept = grid_wide_compact(buf, &s_count, cnt, K, tid, thr);
                }
                const int j = base + tid;
                bool take = false;
                unsigned long long key = ~0ull;
                if (j < T) {
                    int t = 0;                                // the last run starting at or before j: the one that holds point j
#pragma unroll
                    for (int s = 128; s > 0; s >>= 1) t += s_off[t + s] <= j ? s : 0;
                    const size_t p = (size_t)(s_p0[t] + (j - s_off[t]));
                    const float d = pccx_sqdist(q[0], q[1], q[2], sxyz[3 * p], sxyz[3 * p + 1], sxyz[3 * p + 2]);
                    key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)sidx[p];
                    take = key < thr;
                }
                const unsigned long long bal = __ballot(take);
                if (bal) {                                    // wave-uniform
                    int at = 0;
                    if (lane == 0) at = atomicAdd(&s_count, __popcll(bal));
                    at = __shfl(at, 0) + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                    if (take) buf[at] = key;                  // at < count <= ub + 256 <= cap
                }
                ub += 256;
            }
        }
        // every cell visited?  (integers only: this is what ends the loop when no distance ever does)
        if (c[0] - r <= 0 && c[0] + r >= g.G[0] - 1 && c[1] - r <= 0 && c[1] + r >= g.G[1] - 1 && c[2] - r <= 0 && c[2] + r >= g.G[2] - 1) break;
        __syncthreads();
        const int cnt = s_count;
        __syncthreads();
        ub = cnt;
        if (cnt >= K) {
            if (cnt != kept) ub = kept = grid_wide_compact(buf, &s_count, cnt, K, tid, thr);      // thr = the K-th best of all visited
            if (__uint_as_float((unsigned)(thr >> 32)) < grid_face_bound2(g, q, c, r)) break;     // strict: see "same tie rule" above
        }
    }
    __syncthreads();
    const int cnt = s_count;
    __syncthreads();
    if (cnt != kept) grid_wide_compact(buf, &s_count, cnt, K, tid, thr);
    // every cell was visited or K keys lie below the bound: buf[0 .. K) is the answer, ascending (K <= N <= the points visited)
    for (int k = tid; k < K; k += 256) {
        const unsigned long long v = buf[k];
        const int i = (int)(unsigned)v;
        const size_t o = (size_t)qi * K + k;
        if (dists) dists[o] = __uint_as_float((unsigned)(v >> 32));
        if (idx64) idx64[o] = (int64_t)i;
        if (nn) {
            const size_t p = (size_t)inv[(size_t)b * N + min(max(i, 0), N - 1)];      // the same floats as ref[b][i]
            float x = sxyz[3 * p], y = sxyz[3 * p + 1], z = sxyz[3 * p + 2];
            if (patch_scale != 0.f) {
                // grouped_xyz -= centre (compress.py:72); x_patches * (N/N0)^(1/3) (compress.py:108)
                x = __fmul_rn(__fsub_rn(x, q[0]), patch_scale);
                y = __fmul_rn(__fsub_rn(y, q[1]), patch_scale);
                z = __fmul_rn(__fsub_rn(z, q[2]), patch_scale);
            }
            nn[3 * o] = x; nn[3 * o + 1] = y; nn[3 * o + 2] = z;
        }
    }
}

extern "C" int pccx_grid_knn_wide(const float *q, int B, int M, int N, int K, const void *index, void *query_workspace, float *dists,
                                  int64_t *idx, float *nn, float patch_scale, const int32_t *rep, void *stream)
{
    const char *who = "pccx_grid_knn_wide";
    PCCX_CHECK_ARG(q && index && query_workspace, "%s: null pointer", who);
    PCCX_CHECK_ARG(dists || idx || nn, "%s: at least one of dists / idx / nn is needed", who);
    PCCX_CHECK_ARG((((uintptr_t)index | (uintptr_t)query_workspace) & 15) == 0, "%s: the index and the query workspace must be 16-byte aligned", who);
    PCCX_CHECK_ARG(B >= 1 && B <= 65535 && M >= 1 && N >= 1, "%s: bad shape B=%d queries=%d N=%d (1 <= B <= 65535, both clouds non-empty)", who, B, M, N);
    PCCX_CHECK_ARG((long long)B * M < (1ll << 31) && (long long)B * N < (1ll << 31), "%s: B * points must stay below 2^31", who);
    PCCX_CHECK_ARG(K >= 1 && K <= GRID_WIDE_KMAX && K <= N, "%s: need 1 <= K <= min(N,%d), got K=%d N=%d", who, GRID_WIDE_KMAX, K, N);
    const GridLayout L = grid_layout(B, N);
    const char *ws = (const char *)index;
    const int *params = (const int *)(ws + L.params), *cstart = (const int *)(ws + L.cstart), *sidx = (const int *)(ws + L.sidx);
    const float *sxyz = (const float *)(ws + L.sxyz);
    int *inv = (int *)query_workspace;
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)B * N;
    if (nn) hipLaunchKernelGGL(grid_inverse_kernel, dim3(grid_blocks(total, 4096)), dim3(256), 0, st, sidx, N, total, inv);
    hipLaunchKernelGGL(grid_wide_kernel, dim3((unsigned)((long long)B * M)), dim3(256), 0, st, q, B, M, N, params, cstart, L.S, sxyz, sidx,
                       (const int *)inv, K, (const int *)rep, dists, idx, nn, patch_scale);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}
