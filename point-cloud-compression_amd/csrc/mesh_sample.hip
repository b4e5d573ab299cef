// Point clouds sampled from triangle meshes on the GPU ("meshes"): pccx_mesh_sample.
//
// The batch is ragged: verts (V_total, 3) f32 and faces (F_total, 3) int32 hold mesh after mesh, v_off / f_off (B + 1) int64 say where.
// Sample i of mesh b is a function of (mesh b, seeds[b], i) alone and is pinned bit for bit (tests/mesh_cases.py restates it in numpy):
//   a_t = 0.5 sqrt(|(v2 - v1) x (v3 - v1)|^2) in float64, w_t = floor(a_t / a_max 2^40) as uint64, I_t = inclusive prefix, W = I_{F-1};
//   x0..x3 = Philox4x32-10(key = seed, counter = i); target = ((x1 2^32 + x0) W) >> 64; triangle = first t with I_t > target;
//   u = (x2 + 0.5) 2^-32, v = (x3 + 0.5) 2^-32, both reflected when u + v > 1; p = v1 u + v2 v + v3 (1 - (u + v)) in float64 -> float32;
//   normalize: (p - m) / M, m = the mesh's smallest value, M = fl32(largest - m).
// Integer weights make the prefix exact in any summation order, so tiles can be summed apart and scanned afterwards.
//
//   mesh_init_kernel     (1)          clamps the offset tables into one record per mesh, clears its reductions, scans the meshes' tile counts
//   mesh_area_kernel     (G)          256-face tiles over the ragged batch: a_t, and the mesh's largest by an integer max of its bit pattern
//   mesh_weight_kernel   (G)          w_t and the tile's sum
//   mesh_scan_kernel     (B)          exclusive scan of a mesh's tile sums; W
//   mesh_prefix_kernel   (G)          I_t
//   mesh_draw_kernel     (n/256, B)   Philox, the pick (binary search of I), the point; the mesh's smallest and largest value by integer
//                                     atomics on order-preserving keys; status 0 / 1
//   mesh_unit_kernel     (n/256, B)   shift and scale in place; status 2
// G = F_total / 256 + B bounds the sum of ceil(F_b / 256): every grid is a function of (B, F_total, n) alone.  Integer atomics only, so no
// result depends on arrival order; no memset / memcpy: every table is cleared or fully written by a kernel of the call before it is read.
#include "common.h"

#define MESH_THREADS 256
#define MESH_MAX_B 1024
#define MESH_MAX_N (1 << 20)
#define MESH_MAX_F (1 << 22)
#define MESH_INF_BITS 0x7FF0000000000000ull

namespace {

typedef unsigned long long u64;

struct MeshRec {                   // 64 bytes per mesh, written by mesh_init_kernel
    long long fbase, vbase;        // first row of the mesh in faces / verts
    int F, nv;                     // clamped: rows fbase .. + F lie inside faces, vbase .. + nv inside verts; F = 0 for a mesh outside the limits
    u64 amax;                      // bit pattern of the largest a_t (a non-negative double orders as its bits do); MESH_INF_BITS = not finite
    u64 W;
    unsigned kmin, kmax;           // order-preserving keys of the smallest and largest sampled value
    int tile0, pad_[3];
};

static inline size_t mesh_tiles(long long F_total, int B) { return (size_t)(F_total / MESH_THREADS) + (size_t)B; }

// inclusive prefix of v over the 256 threads (red: 4 words of LDS); every thread also gets the total
__device__ __forceinline__ u64 mesh_block_incl(u64 v, u64 *red, u64 &total)
{
    const int lane = pccx_lane(), w = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        u64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                   // red may still be read from the call before
    if (lane == 63) red[w] = inc;
    __syncthreads();
    u64 before = 0, all = 0;
#pragma unroll
    for (int j = 0; j < MESH_THREADS / 64; ++j) {
        u64 t = red[j];
        if (j < w) before += t;
        all += t;
    }
    total = all;
    return before + inc;
}

// the mesh whose tiles hold this one: the last b with tile_prefix[b] <= tile, or -1 (workgroup-uniform)
__device__ __forceinline__ int mesh_of_tile(const int32_t *__restrict__ tp, int B, int tile)
{
    if (tile < tp[0] || tile >= tp[B]) return -1;
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tp[mid] <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// rows of mesh j, clamped into the two stores; F = 0 for a mesh without a vertex or with more than MESH_MAX_F faces
__device__ __forceinline__ void mesh_clamp(const int64_t *__restrict__ v_off, const int64_t *__restrict__ f_off, long long V_total, long long F_total,
                                           int j, long long &fb, long long &vb, int &F, int &nv)
{
    fb = min(max((long long)f_off[j], 0ll), F_total);
    const long long fe = min(max((long long)f_off[j + 1], fb), F_total);
    vb = min(max((long long)v_off[j], 0ll), V_total);
    const long long ve = min(max((long long)v_off[j + 1], vb), V_total);
    nv = (int)min(ve - vb, 2147483647ll);
    F = (fe - fb > MESH_MAX_F || nv < 1) ? 0 : (int)(fe - fb);
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_init_kernel(const int64_t *__restrict__ v_off, const int64_t *__restrict__ f_off, long long V_total,
                                                                 long long F_total, int B, long long G, MeshRec *__restrict__ rec,
                                                                 int32_t *__restrict__ tp)
{
    __shared__ u64 red[4];
    const int per = (B + MESH_THREADS - 1) / MESH_THREADS, j0 = min((int)threadIdx.x * per, B), j1 = min(j0 + per, B);
    long long fb, vb;
    int F, nv;
    u64 sum = 0, total;
    for (int j = j0; j < j1; ++j) {
        mesh_clamp(v_off, f_off, V_total, F_total, j, fb, vb, F, nv);
        sum += (u64)((F + MESH_THREADS - 1) / MESH_THREADS);
    }
    u64 run = mesh_block_incl(sum, red, total) - sum;
    for (int j = j0; j < j1; ++j) {
        mesh_clamp(v_off, f_off, V_total, F_total, j, fb, vb, F, nv);
        const u64 end = run + (u64)((F + MESH_THREADS - 1) / MESH_THREADS);
        MeshRec r;
        r.fbase = fb, r.vbase = vb, r.nv = nv;
        r.F = end <= (u64)G ? F : 0;                   // offsets that overlap could ask for more tiles than the grid and the tile table hold
        r.amax = 0ull, r.W = 0ull, r.kmin = 0xFFFFFFFFu, r.kmax = 0u, r.tile0 = (int)run;
        r.pad_[0] = r.pad_[1] = r.pad_[2] = 0;
        rec[j] = r;
        tp[j] = (int)run;
        run = end;
    }
    if (threadIdx.x == 0) tp[B] = (int)total;          // <= 1024 * 2^22 / 256 = 2^24
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_area_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                                 MeshRec *__restrict__ rec, const int32_t *__restrict__ tp, int B,
                                                                 double *__restrict__ area)
{
    const int tile = blockIdx.x, b = mesh_of_tile(tp, B, tile);
    if (b < 0) return;
    const long long fbase = rec[b].fbase, vbase = rec[b].vbase;
    const int F = rec[b].F, nv = rec[b].nv;
    const int t = (tile - tp[b]) * MESH_THREADS + (int)threadIdx.x;
    u64 bits = 0ull;
    if (t < F) {
        const int32_t *f = faces + 3 * (fbase + t);
        const float *p1 = verts + 3 * (vbase + min(max(f[0], 0), nv - 1));
        const float *p2 = verts + 3 * (vbase + min(max(f[1], 0), nv - 1));
        const float *p3 = verts + 3 * (vbase + min(max(f[2], 0), nv - 1));
        const double ux = (double)p2[0] - (double)p1[0], uy = (double)p2[1] - (double)p1[1], uz = (double)p2[2] - (double)p1[2];
        const double vx = (double)p3[0] - (double)p1[0], vy = (double)p3[1] - (double)p1[1], vz = (double)p3[2] - (double)p1[2];
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        const double a = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
        area[fbase + t] = a;
        bits = a < __builtin_huge_val() ? (u64)__double_as_longlong(a) : MESH_INF_BITS;   // NaN compares false: flagged as infinity is
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(bits, o, 64);
        bits = other > bits ? other : bits;
    }
    if (pccx_lane() == 0 && bits) atomicMax(&rec[b].amax, bits);
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_weight_kernel(const MeshRec *__restrict__ rec, const int32_t *__restrict__ tp, int B,
                                                                   const double *__restrict__ area, u64 *__restrict__ wgt, u64 *__restrict__ tsum)
{
    __shared__ u64 red[4];
    const int tile = blockIdx.x, b = mesh_of_tile(tp, B, tile);
    if (b < 0) return;
    const MeshRec r = rec[b];
    const int t = (tile - tp[b]) * MESH_THREADS + (int)threadIdx.x;
    u64 w = 0ull, total;
    if (t < r.F) {
        if (r.amax > 0ull && r.amax < MESH_INF_BITS) w = (u64)floor(area[r.fbase + t] / __longlong_as_double((long long)r.amax) * 0x1p40);
        wgt[r.fbase + t] = w;
    }
    mesh_block_incl(w, red, total);
    if (threadIdx.x == 0) tsum[tile] = total;
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_scan_kernel(MeshRec *__restrict__ rec, u64 *__restrict__ tsum)
{
    __shared__ u64 red[4];
    const int b = blockIdx.x, nt = (rec[b].F + MESH_THREADS - 1) / MESH_THREADS;
    u64 *c = tsum + rec[b].tile0;
    const int per = (nt + MESH_THREADS - 1) / MESH_THREADS, j0 = min((int)threadIdx.x * per, nt), j1 = min(j0 + per, nt);
    u64 sum = 0ull, total;
    for (int j = j0; j < j1; ++j) sum += c[j];
    u64 run = mesh_block_incl(sum, red, total) - sum;
    for (int j = j0; j < j1; ++j) {
        const u64 v = c[j];
        c[j] = run;
        run += v;
    }
    if (threadIdx.x == 0) rec[b].W = total;
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_prefix_kernel(const MeshRec *__restrict__ rec, const int32_t *__restrict__ tp, int B,
                                                                   const u64 *__restrict__ wgt, const u64 *__restrict__ tsum, u64 *__restrict__ incl)
{
    __shared__ u64 red[4];
    const int tile = blockIdx.x, b = mesh_of_tile(tp, B, tile);
    if (b < 0) return;
    const long long fbase = rec[b].fbase;
    const int F = rec[b].F;
    const int t = (tile - tp[b]) * MESH_THREADS + (int)threadIdx.x;
    u64 total;
    const u64 inc = mesh_block_incl(t < F ? wgt[fbase + t] : 0ull, red, total);
    if (t < F) incl[fbase + t] = tsum[tile] + inc;
}

__device__ __forceinline__ void mesh_philox(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned x[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

// a float's bits -> a key that orders as the float does (-0 below +0), and back
__device__ __forceinline__ unsigned mesh_key(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mesh_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__global__ __launch_bounds__(MESH_THREADS) void mesh_draw_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                                 MeshRec *__restrict__ rec, const u64 *__restrict__ incl,
                                                                 const int64_t *__restrict__ seeds, int n, float *__restrict__ out,
                                                                 int32_t *__restrict__ status)
{
    const int b = blockIdx.y, i = blockIdx.x * MESH_THREADS + (int)threadIdx.x;
    const long long fbase = rec[b].fbase, vbase = rec[b].vbase;
    const int F = rec[b].F, nv = rec[b].nv;
    const u64 W = rec[b].W;
    if (blockIdx.x == 0 && threadIdx.x == 0) status[b] = W > 0ull ? 0 : 1;
    unsigned kmin = 0xFFFFFFFFu, kmax = 0u;
    if (i < n) {
        const float nan = __uint_as_float(0x7FC00000u);
        float px = nan, py = nan, pz = nan;
        if (W > 0ull) {
            const u64 s = (u64)seeds[b];
            unsigned x[4];
            mesh_philox((unsigned)s, (unsigned)(s >> 32), (unsigned)i, 0u, 0u, 0u, x);
            const u64 target = __umul64hi(((u64)x[1] << 32) | x[0], W);            // < W = incl[F - 1]
            const u64 *I = incl + fbase;
            int lo = 0, hi = F - 1;
            while (lo < hi) {                                                      // the first t with I_t > target
                const int mid = (lo + hi) >> 1;
                if (I[mid] > target) hi = mid;
                else lo = mid + 1;
            }
            const int32_t *f = faces + 3 * (fbase + lo);
            const float *p1 = verts + 3 * (vbase + min(max(f[0], 0), nv - 1));
            const float *p2 = verts + 3 * (vbase + min(max(f[1], 0), nv - 1));
            const float *p3 = verts + 3 * (vbase + min(max(f[2], 0), nv - 1));
            double u = ((double)x[2] + 0.5) * 0x1p-32, v = ((double)x[3] + 0.5) * 0x1p-32;
            if (u + v > 1.0) u = 1.0 - u, v = 1.0 - v;
            const double w3 = 1.0 - (u + v);
            px = (float)(((double)p1[0] * u + (double)p2[0] * v) + (double)p3[0] * w3);
            py = (float)(((double)p1[1] * u + (double)p2[1] * v) + (double)p3[1] * w3);
            pz = (float)(((double)p1[2] * u + (double)p2[2] * v) + (double)p3[2] * w3);
            const unsigned kx = mesh_key(px), ky = mesh_key(py), kz = mesh_key(pz);
            kmin = min(kx, min(ky, kz)), kmax = max(kx, max(ky, kz));
        }
        float *o = out + 3 * ((size_t)b * n + i);
        o[0] = px, o[1] = py, o[2] = pz;
    }
    if (W == 0ull) return;                                                         // workgroup-uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kmin = min(kmin, (unsigned)__shfl_xor(kmin, o, 64));
        kmax = max(kmax, (unsigned)__shfl_xor(kmax, o, 64));
    }
    if (pccx_lane() == 0 && kmin <= kmax) {                                        // a wave behind n has nothing to say
        atomicMin(&rec[b].kmin, kmin);
        atomicMax(&rec[b].kmax, kmax);
    }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_unit_kernel(const MeshRec *__restrict__ rec, int n, float *__restrict__ out,
                                                                 int32_t *__restrict__ status)
{
    const int b = blockIdx.y, i = blockIdx.x * MESH_THREADS + (int)threadIdx.x;
    if (rec[b].W == 0ull) return;                                                  // status 1: the rows stay NaN
    const float m = mesh_unkey(rec[b].kmin), M = mesh_unkey(rec[b].kmax) - m;
    if (blockIdx.x == 0 && threadIdx.x == 0 && M == 0.f) status[b] = 2;
    if (i < n) {
        float *o = out + 3 * ((size_t)b * n + i);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float q = o[c] - m;
            o[c] = M == 0.f ? q : q / M;
        }
    }
}

// byte offsets of the workspace's parts: a_t, w_t, I_t, tile sums, records, tile prefix
struct MeshLayout {
    size_t area, wgt, incl, tsum, rec, tp, end;
    MeshLayout(int B, long long F_total)
    {
        const size_t F = (size_t)F_total;
        area = 0, wgt = 8 * F, incl = 16 * F, tsum = 24 * F;
        rec = tsum + 8 * mesh_tiles(F_total, B);
        tp = rec + sizeof(MeshRec) * (size_t)B;
        end = (tp + 4 * ((size_t)B + 1) + 7) / 8 * 8;
    }
};

}  // namespace

extern "C" size_t pccx_mesh_sample_workspace_bytes(int B, int64_t F_total, int n)
{
    if (B < 0 || F_total < 0 || n < 0) return 0;
    return MeshLayout(B, F_total).end;
}

extern "C" int pccx_mesh_sample(const float *verts, int64_t V_total, const int32_t *faces, int64_t F_total, const int64_t *v_off,
                                const int64_t *f_off, const int64_t *seeds, int B, int n, int normalize, float *out, int32_t *status,
                                void *workspace, void *stream)
{
    PCCX_CHECK_ARG(B >= 0 && B <= MESH_MAX_B, "pccx_mesh_sample: B=%d meshes, at most MESH_MAX_B = %d per call", B, MESH_MAX_B);
    PCCX_CHECK_ARG(n >= 1 && n <= MESH_MAX_N, "pccx_mesh_sample: n=%d, a cloud holds 1..MESH_MAX_N = %d samples", n, MESH_MAX_N);
    PCCX_CHECK_ARG(V_total >= 1 && F_total >= 1 && F_total <= (int64_t)MESH_MAX_B * MESH_MAX_F, "pccx_mesh_sample: bad store V_total=%lld F_total=%lld",
                   (long long)V_total, (long long)F_total);
    PCCX_CHECK_ARG(normalize == 0 || normalize == 1, "pccx_mesh_sample: normalize=%d, 0 (raw) or 1 (unit) is expected", normalize);
    if (B == 0) return PCCX_OK;
    PCCX_CHECK_ARG(verts && faces && v_off && f_off && seeds && out && status && workspace, "pccx_mesh_sample: null pointer");
    PCCX_CHECK_ARG((uintptr_t)workspace % 8 == 0, "pccx_mesh_sample: the workspace must be 8-byte aligned");
    static_assert(sizeof(MeshRec) == 64, "MeshRec is 64 bytes");
    hipStream_t st = (hipStream_t)stream;
    const MeshLayout L(B, F_total);
    uint8_t *ws = (uint8_t *)workspace;
    double *area = (double *)(ws + L.area);
    u64 *wgt = (u64 *)(ws + L.wgt), *incl = (u64 *)(ws + L.incl), *tsum = (u64 *)(ws + L.tsum);
    MeshRec *rec = (MeshRec *)(ws + L.rec);
    int32_t *tp = (int32_t *)(ws + L.tp);
    const long long G = (long long)mesh_tiles(F_total, B);
    const dim3 block(MESH_THREADS), tiles((unsigned)G), draws((unsigned)((n + MESH_THREADS - 1) / MESH_THREADS), (unsigned)B);
    hipLaunchKernelGGL(mesh_init_kernel, dim3(1), block, 0, st, v_off, f_off, (long long)V_total, (long long)F_total, B, G, rec, tp);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_area_kernel, tiles, block, 0, st, verts, faces, rec, (const int32_t *)tp, B, area);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_weight_kernel, tiles, block, 0, st, (const MeshRec *)rec, (const int32_t *)tp, B, (const double *)area, wgt, tsum);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(B), block, 0, st, rec, tsum);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_prefix_kernel, tiles, block, 0, st, (const MeshRec *)rec, (const int32_t *)tp, B, (const u64 *)wgt, (const u64 *)tsum, incl);
    PCCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_draw_kernel, draws, block, 0, st, verts, faces, rec, (const u64 *)incl, seeds, n, out, status);
    PCCX_CHECK_LAUNCH();
    if (normalize) {
        hipLaunchKernelGGL(mesh_unit_kernel, draws, block, 0, st, (const MeshRec *)rec, n, out, status);
        PCCX_CHECK_LAUNCH();
    }
    return PCCX_OK;
}
