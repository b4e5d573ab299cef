// eval_metrics.hip -- the evaluation metrics of eval.py over ragged batches: clouds of different sizes in one
// padded slab, cloud b in the first n[b] rows of its slab.  Bounding box, PCA normals, point-to-point and point-to-plane error from ONE
// all-pairs scan, and per-cloud mean / variance in a fixed order.
//
// The conventions are nn_dist_n_kernel's (knn.hip): every count is (B) int32 ON THE DEVICE and is clamped into its capacity where it is
// read; a row behind a count is never loaded (pad_clouds leaves NaN there), an output behind a count stays unwritten, and a cloud with a
// zero count forms no address into its slab.  The arithmetic is the dense kernels' (nn_scan.h), so cloud b's rows are bit for bit those
// of the dense entry points on the unpadded cloud.
#include "common.h"
#include "nn_scan.h"

// ------------------------------------------------------------------------------------------
// pccx_minmax_n: one workgroup per cloud.  fminf / fmaxf are exact and commutative, so the order of the reduction does not matter: the
// result is amin / amax of the unpadded cloud.  A zero count gives the identities (+inf, -inf).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void minmax_n_kernel(const float *__restrict__ X, int P_max, const int32_t *__restrict__ p, float *__restrict__ out)
{
    __shared__ float red[6][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int pb = min(max(p[b], 0), P_max);
    const float *xp = X + (size_t)b * P_max * 3;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < pb; i += 256)
#pragma unroll
        for (int a = 0; a < 3; ++a) { const float v = xp[3 * i + a]; lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v); }
#pragma unroll
    for (int a = 0; a < 3; ++a) { red[a][tid] = lo[a]; red[3 + a][tid] = hi[a]; }
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if (tid < o)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                red[a][tid] = fminf(red[a][tid], red[a][tid + o]);
                red[3 + a][tid] = fmaxf(red[3 + a][tid], red[3 + a][tid + o]);
            }
        __syncthreads();
    }
    if (tid < 6) out[(size_t)b * 6 + tid] = red[tid][0];
}

extern "C" int pccx_minmax_n(const float *X, int B, int P_max, const int32_t *p, float *out, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    PCCX_CHECK_ARG(X && p && out, "pccx_minmax_n: null pointer");
    PCCX_CHECK_ARG(B >= 0 && B <= 65535 && P_max >= 1, "pccx_minmax_n: bad shape B=%d P_max=%d", B, P_max);
    hipLaunchKernelGGL(minmax_n_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, X, P_max, p, out);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

// ------------------------------------------------------------------------------------------
// pccx_query_rep_n: the `rep` table that keeps pccx_knn_list_n from searching padded queries.  Query i of cloud b is its own
// representative while i < n[b]; every query behind the count names query 0 of its cloud, and the kNN kernels leave on rep[p] != p.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void query_rep_n_kernel(const int32_t *__restrict__ n, int M, int32_t *__restrict__ rep)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int nb = min(max(n[b], 0), M);
    rep[(size_t)b * M + i] = i < nb ? b * M + i : b * M;
}

extern "C" int pccx_query_rep_n(const int32_t *n, int B, int M, int32_t *rep, void *stream)
{
    if (B == 0 || M == 0) return PCCX_OK;
    PCCX_CHECK_ARG(n && rep, "pccx_query_rep_n: null pointer");
    PCCX_CHECK_ARG(B >= 0 && B <= 65535 && M >= 0 && (long long)B * M <= 0x7fffffffll, "pccx_query_rep_n: bad shape B=%d M=%d", B, M);
    hipLaunchKernelGGL(query_rep_n_kernel, dim3((M + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, n, M, rep);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

// ------------------------------------------------------------------------------------------
// pccx_estimate_normals_n: normals_pca_kernel over per-cloud counts.  Row i < n[b] reads its K neighbour indices (written by
// pccx_knn_list_n for exactly those rows, each inside [0, n[b])) and the points they name; the index rows behind the count, which that
// search leaves unwritten, are never read.
// ------------------------------------------------------------------------------------------
__global__ void normals_pca_n_kernel(const float *__restrict__ xyz, int N_max, const int32_t *__restrict__ n, const int64_t *__restrict__ nbr,
                                     int K, float *__restrict__ normals)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int nb = min(max(n[b], 0), N_max);
    if (i >= nb) return;
    normals_pca_point(xyz + (size_t)b * N_max * 3, nbr + ((size_t)b * N_max + i) * K, K, normals + ((size_t)b * N_max + i) * 3);
}

extern "C" int pccx_estimate_normals_n(const float *xyz, int B, int N_max, const int32_t *n, const int64_t *nbr, int K, float *normals,
                                       void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    PCCX_CHECK_ARG(xyz && n && nbr && normals, "pccx_estimate_normals_n: null pointer");
    PCCX_CHECK_ARG(B >= 0 && N_max >= 1 && K >= 1 && B <= 65535, "pccx_estimate_normals_n: bad shape");
    hipLaunchKernelGGL(normals_pca_n_kernel, dim3((N_max + 127) / 128, B), dim3(128), 0, (hipStream_t)stream, xyz, N_max, n, nbr, K, normals);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

// ------------------------------------------------------------------------------------------
// pccx_point_errors_n: D1 and D2 from one scan.  nn_dist_scan_core<true, XPT> leaves every query's minimum and first argmin in registers;
// the epilogue writes the squared distance and, where normals are given, plane_err_kernel's value for that argmin -- the int32 argmin
// table of the two-kernel form is never written.  Without normals the scan runs without the argmin (the minima are the same floats).
// ------------------------------------------------------------------------------------------
template <bool PLANE, int XPT>
__global__ __launch_bounds__(256) void point_errors_n_kernel(const float *__restrict__ X, int P_max, const int32_t *__restrict__ p,
                                                             const float *__restrict__ Y, const float *__restrict__ nY, int Q_max,
                                                             const int32_t *__restrict__ q, float *__restrict__ d2, float *__restrict__ plane)
{
    const int b = blockIdx.y, tid = threadIdx.x;
    const int pb = min(max(p[b], 0), P_max), qb = min(max(q[b], 0), Q_max);
    if ((int)blockIdx.x * (256 * XPT) >= pb || qb == 0) return;
    const size_t row = (size_t)b * P_max;
    const float *xp = X + row * 3, *yp = Y + (size_t)b * Q_max * 3;
    float best[XPT];
    int bi[XPT];
    nn_dist_scan_core<PLANE, XPT>(xp, pb, yp, 0, qb, best, bi);
#pragma unroll
    for (int j = 0; j < XPT; ++j) {
        const int i = blockIdx.x * (256 * XPT) + j * 256 + tid;
        if (i < pb) {
            d2[row + i] = best[j];
            if (PLANE) {
                // no reference was strictly nearer than +inf (a NaN among the coordinates: outside the contract): no row to project on
                const int k = bi[j];
                plane[row + i] = k >= 0 && k < qb ? plane_err_value(xp + 3 * (size_t)i, yp + 3 * (size_t)k, nY + ((size_t)b * Q_max + k) * 3)
                                                  : __uint_as_float(0x7FC00000u);
            }
        }
    }
}

extern "C" int pccx_point_errors_n(const float *X, int B, int P_max, const int32_t *p, const float *Y, const float *normals_Y, int Q_max,
                                   const int32_t *q, float *d2, float *plane, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    PCCX_CHECK_ARG(X && Y && p && q && d2, "pccx_point_errors_n: null pointer");
    PCCX_CHECK_ARG(!normals_Y == !plane, "pccx_point_errors_n: normals_Y and plane come together");
    PCCX_CHECK_ARG(B >= 0 && P_max >= 1 && Q_max >= 1, "pccx_point_errors_n: bad shape");
    PCCX_CHECK_ARG(B <= 65535, "pccx_point_errors_n: B=%d > 65535 unsupported", B);
    const bool small = (long long)B * ((P_max + 1023) / 1024) < 512;      // as pccx_nn_dist_n
    const int xpt = small ? 1 : 4;
    const int gx = (P_max + 256 * xpt - 1) / (256 * xpt);
    hipStream_t st = (hipStream_t)stream;
    if (plane) {
        if (small) hipLaunchKernelGGL((point_errors_n_kernel<true, 1>), dim3(gx, B), dim3(256), 0, st, X, P_max, p, Y, normals_Y, Q_max, q, d2, plane);
        else hipLaunchKernelGGL((point_errors_n_kernel<true, 4>), dim3(gx, B), dim3(256), 0, st, X, P_max, p, Y, normals_Y, Q_max, q, d2, plane);
    } else {
        if (small) hipLaunchKernelGGL((point_errors_n_kernel<false, 1>), dim3(gx, B), dim3(256), 0, st, X, P_max, p, Y, normals_Y, Q_max, q, d2, plane);
        else hipLaunchKernelGGL((point_errors_n_kernel<false, 4>), dim3(gx, B), dim3(256), 0, st, X, P_max, p, Y, normals_Y, Q_max, q, d2, plane);
    }
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

// ------------------------------------------------------------------------------------------
// pccx_mean_var_n: mean and population variance of the first p[b] entries of row b, two passes in fp64 (the mean, then the centred
// squares).  One workgroup per cloud; thread t adds the entries t, t + 256, t + 512, ... in that order, then a fixed tree over the 256
// partial sums.  The order is a function of p[b] alone -- no atomics, no dependence on the batch, the cloud's position or P_max.
// A zero count gives NaN for both (0 / 0), without a load.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double mean_var_block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();                                   // red may still be read from the call before
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void mean_var_n_kernel(const float *__restrict__ v, int P_max, const int32_t *__restrict__ p, double *__restrict__ out)
{
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int pb = min(max(p[b], 0), P_max);
    const float *vp = v + (size_t)b * P_max;
    double s = 0.0;
    for (int i = tid; i < pb; i += 256) s += (double)vp[i];
    const double mean = mean_var_block_sum(s, red) / (double)pb;
    double c = 0.0;
    for (int i = tid; i < pb; i += 256) {
        const double d = (double)vp[i] - mean;
        c += d * d;
    }
    const double var = mean_var_block_sum(c, red) / (double)pb;
    if (tid == 0) { out[(size_t)b * 2] = mean; out[(size_t)b * 2 + 1] = var; }
}

extern "C" int pccx_mean_var_n(const float *v, int B, int P_max, const int32_t *p, double *out, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    PCCX_CHECK_ARG(v && p && out, "pccx_mean_var_n: null pointer");
    PCCX_CHECK_ARG(B >= 0 && B <= 65535 && P_max >= 1, "pccx_mean_var_n: bad shape B=%d P_max=%d", B, P_max);
    hipLaunchKernelGGL(mean_var_n_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, v, P_max, p, out);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}
