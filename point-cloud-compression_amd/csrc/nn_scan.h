// Device bodies shared by knn.hip and eval_metrics.hip: the LDS-tiled all-pairs nearest-neighbour scan, the PCA normal of one point
// and the point-to-plane error of one pair.  Each is stated once, so the dense and the ragged kernels agree bit for bit.
#pragma once
#include <math.h>

#include "common.h"

// ------------------------------------------------------------------------------------------
// nn_dist: LDS-tiled all-pairs min-reduce.  A 256-thread workgroup owns 1024 query points
// (4 per thread, registers) and streams the other cloud through LDS in tiles of 1024 points
// (12 KiB); every lane reads the same LDS address (broadcast, conflict-free), so one 12-byte LDS
// read feeds 4 distance evaluations.  Algorithmic HBM bytes: 12(P+Q) + 8P per cloud; the P*Q pair
// work is VALU-bound (8 flops/pair).
// ------------------------------------------------------------------------------------------
#define NND_TILE 1024
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Two reference points per step: the three differences, squares and the two adds run as packed fp32
// (v_pk_add_f32 / v_pk_mul_f32, no contraction: the file is built with -ffp-contract=off), the same
// operation sequence per pair as pccx_sqdist.  Without the argmin the update is one v_min3_f32.
// XPT queries per thread: 4 (1024 per workgroup) for the evaluation batches; 1 when the batch is too small to fill the chip that way
// (the training step's 4 clouds: 32 workgroups become 128).  A query's scan over Y is the same sequence either way.
// One workgroup's share of a cloud: its 256 XPT queries of the P rows at xp against the references [q_begin, q_end) of yp.  The minima
// (and, with WANT_NN, the first argmins) of query blockIdx.x * 256 XPT + j * 256 + tid come back in best[j] / bi[j], still in registers.
template <bool WANT_NN, int XPT>
__device__ __forceinline__ void nn_dist_scan_core(const float *__restrict__ xp, int P, const float *__restrict__ yp, int q_begin, int q_end,
                                                  float (&best)[XPT], int (&bi)[XPT])
{
    __shared__ __attribute__((aligned(8))) float tyx[NND_TILE], tyy[NND_TILE], tyz[NND_TILE];
    const int tid = threadIdx.x;
    float x[XPT][3];
#pragma unroll
    for (int j = 0; j < XPT; ++j) {
        int i = blockIdx.x * (256 * XPT) + j * 256 + tid;
        int ii = i < P ? i : P - 1;
        x[j][0] = xp[3 * ii]; x[j][1] = xp[3 * ii + 1]; x[j][2] = xp[3 * ii + 2];
        best[j] = INFINITY; bi[j] = -1;
    }
    for (int base = q_begin; base < q_end; base += NND_TILE) {
        const int cnt = q_end - base < NND_TILE ? q_end - base : NND_TILE;
        const int cnt2 = (cnt + 1) & ~1;                  // an odd tail repeats its last point: no effect on min / first argmin
        __syncthreads();
        for (int t = tid; t < cnt2; t += 256) {
            const size_t src = (size_t)(base + (t < cnt ? t : cnt - 1)) * 3;
            tyx[t] = yp[src]; tyy[t] = yp[src + 1]; tyz[t] = yp[src + 2];
        }
        __syncthreads();
        for (int t = 0; t < cnt2; t += 2) {
            const f32x2 yx = *(const f32x2 *)&tyx[t], yy = *(const f32x2 *)&tyy[t], yz = *(const f32x2 *)&tyz[t];
#pragma unroll
            for (int j = 0; j < XPT; ++j) {
                const f32x2 dx = x[j][0] - yx, dy = x[j][1] - yy, dz = x[j][2] - yz;
                f32x2 d = dx * dx;
                d = d + dy * dy;
                d = d + dz * dz;
                if (WANT_NN) {
                    if (d.x < best[j]) { best[j] = d.x; bi[j] = base + t; }
                    if (d.y < best[j]) { best[j] = d.y; bi[j] = base + t + 1; }
                } else
                    best[j] = fminf(fminf(best[j], d.x), d.y);
            }
        }
    }
}

// The scan with its plain epilogue: d2 / nn are the cloud's output rows.  nn_dist_kernel and nn_dist_n_kernel differ only in where P and
// the range come from.
template <bool WANT_NN, int XPT>
__device__ __forceinline__ void nn_dist_scan(const float *__restrict__ xp, int P, const float *__restrict__ yp, int q_begin, int q_end,
                                             float *__restrict__ d2, int32_t *__restrict__ nn)
{
    const int tid = threadIdx.x;
    float best[XPT];
    int bi[XPT];
    nn_dist_scan_core<WANT_NN, XPT>(xp, P, yp, q_begin, q_end, best, bi);
#pragma unroll
    for (int j = 0; j < XPT; ++j) {
        int i = blockIdx.x * (256 * XPT) + j * 256 + tid;
        if (i < P) {
            d2[i] = best[j];
            if (WANT_NN) nn[i] = bi[j];
        }
    }
}

// ------------------------------------------------------------------------------------------
// D2 (point-to-plane) support for eval.py:58-60,73-81.
//   normals_pca_point : PCA of one point's K nearest neighbours (open3d estimate_normals with
//                       KDTreeSearchParamKNN): fp64 covariance, analytic symmetric 3x3 eigen-solve,
//                       eigenvector of the smallest eigenvalue.  The sign is arbitrary (as open3d's
//                       unoriented normals); D2 squares the projection.  PARITY UNPINNED vs open3d.
//   plane_err_value   : ((x - y) . n_y)^2 for a reconstructed x and its nearest original y.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void cross3(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// p: the cloud's points; nb: the K neighbour indices of the point; o: its normal (3 floats)
__device__ __forceinline__ void normals_pca_point(const float *__restrict__ p, const int64_t *__restrict__ nb, int K, float *__restrict__ o)
{
    double m[3] = {0, 0, 0};
    for (int k = 0; k < K; ++k)
        for (int a = 0; a < 3; ++a) m[a] += (double)p[3 * nb[k] + a];
    for (int a = 0; a < 3; ++a) m[a] /= K;
    double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
    for (int k = 0; k < K; ++k) {
        const double x = (double)p[3 * nb[k]] - m[0], y = (double)p[3 * nb[k] + 1] - m[1], z = (double)p[3 * nb[k] + 2] - m[2];
        c00 += x * x; c01 += x * y; c02 += x * z; c11 += y * y; c12 += y * z; c22 += z * z;
    }
    c00 /= K; c01 /= K; c02 /= K; c11 /= K; c12 /= K; c22 /= K;
    // smallest eigenvalue of the symmetric matrix (trigonometric closed form), on a scale-normalised copy
    const double scale = fmax(fmax(fabs(c00), fabs(c11)), fmax(fabs(c22), fmax(fabs(c01), fmax(fabs(c02), fabs(c12)))));
    double n[3] = {0, 0, 1};
    if (scale > 0) {
        const double a00 = c00 / scale, a01 = c01 / scale, a02 = c02 / scale, a11 = c11 / scale, a12 = c12 / scale, a22 = c22 / scale;
        const double q = (a00 + a11 + a22) / 3;
        const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
        const double p2 = (a00 - q) * (a00 - q) + (a11 - q) * (a11 - q) + (a22 - q) * (a22 - q) + 2 * p1;
        double lam = q;
        if (p2 > 0) {
            const double pp = sqrt(p2 / 6);
            const double b00 = (a00 - q) / pp, b01 = a01 / pp, b02 = a02 / pp, b11 = (a11 - q) / pp, b12 = a12 / pp, b22 = (a22 - q) / pp;
            double r = (b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02)) / 2;
            r = r < -1 ? -1 : (r > 1 ? 1 : r);
            const double phi = acos(r) / 3;
            lam = q + 2 * pp * cos(phi + 2.0943951023931953);       // smallest eigenvalue (phi + 2*pi/3)
        }
        // eigenvector: the largest cross product of two rows of (A - lam I)
        const double r0[3] = {a00 - lam, a01, a02}, r1[3] = {a01, a11 - lam, a12}, r2[3] = {a02, a12, a22 - lam};
        double c0[3], c1[3], c2[3];
        cross3(r0, r1, c0); cross3(r0, r2, c1); cross3(r1, r2, c2);
        const double d0 = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2];
        const double d1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2];
        const double d2 = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2];
        const double *best = d0 >= d1 && d0 >= d2 ? c0 : (d1 >= d2 ? c1 : c2);
        const double dm = fmax(d0, fmax(d1, d2));
        if (dm > 0) {
            const double inv = 1.0 / sqrt(dm);
            n[0] = best[0] * inv; n[1] = best[1] * inv; n[2] = best[2] * inv;
        }
    }
    o[0] = (float)n[0]; o[1] = (float)n[1]; o[2] = (float)n[2];
}

// x, y, n: three floats each
__device__ __forceinline__ float plane_err_value(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ n)
{
    const double d = (double)(x[0] - y[0]) * n[0] + (double)(x[1] - y[1]) * n[1] + (double)(x[2] - y[2]) * n[2];
    return (float)(d * d);
}
