// Raw PLY vertex records -> float32 x y z rows on the GPU: pccx_ply_unpack.
//
// The host threads of hostio.hip put every file's vertex block, as it is in the file, at a 16-byte-aligned offset of one staging
// buffer; one copy brings it to the device.  Here cloud b's n[b] records of stride[b] bytes become rows dst_row[b] .. dst_row[b] + n[b]
// of out (rows, 3) f32, and rows n[b] .. cap[b] the quiet NaN of codec.pad_clouds: one table serves the padded slab (dst_row = b *
// N_cap, cap = N_cap) and the packed store of codec.pack_clouds (dst_row = offsets[b], cap = n[b]).
//
// Grid: flat over 256-row tiles, tile_prefix (B + 1) int32 = exclusive prefix of ceil(cap[b] / 256); a workgroup finds its cloud by
// a binary search of the prefix, so a room of a million points and a scan of 300 share the chip, and no bound is a maximum over the
// batch.  Table row (PLY_DEV_ROW int64): source byte offset, stride, byte offset of x y z, type code of x y z (ply_host.h), big
// endian, n, dst_row, cap.  Every field is clamped where it is read: a row that does not describe records inside the staging buffer
// and rows inside out unpacks fewer records or none, it never forms an address outside either.
//
// A tile's records are one span of 256 * stride bytes that starts anywhere.  Up to PLY_STAGE_STRIDE = 64 bytes per record the span is
// loaded by 16-byte-aligned 16-byte loads (one per lane and round) into LDS, 16 416 bytes per workgroup -- with the 3 072 bytes the
// output rows pass through, eight workgroups fit the 160 KiB of a CU, as many as its wave slots hold -- and each lane assembles its
// three fields from two or three LDS words (v_alignbit), never from a misaligned float or double pointer.  The converted rows go
// through LDS once more, so that every wave stores 64 consecutive words per instruction.  Longer records (a PLY with dozens of properties) would stage mostly bytes nobody reads: their fields are
// assembled from single-byte global loads.  Conversion is numpy's astype(float32): float32 is a bit copy (NaN payloads included),
// float64 / int32 / uint32 round to nearest even (v_cvt_f32_*), the 8- and 16-bit types are exact.
#include "common.h"
#include "ply_host.h"

#define PLY_THREADS 256
#define PLY_STAGE_STRIDE 64
#define PLY_LDS_QUADS (PLY_THREADS * PLY_STAGE_STRIDE / 16 + 2)      // the span, its 15 bytes of misalignment, and the word a field's last alignbit reads
#define PLY_DEV_ROW 12

namespace {

struct PlyCloud {
    long long src, stride, n, dst, cap;
    int off[3], type[3];
    bool big;
};

__device__ __forceinline__ int ply_size_of(int type)
{
    return type <= PLY_U1 ? 1 : type <= PLY_U2 ? 2 : type <= PLY_F4 ? 4 : 8;
}

// Row b of the table, clamped: afterwards 0 <= n <= cap, rows dst .. dst + cap lie inside out, records 0 .. n inside the staging
// buffer, and every field inside its record.  A row that cannot be made so gets n = 0 (its rows become NaN) or cap = 0 (nothing).
__device__ __forceinline__ PlyCloud ply_cloud(const int64_t *__restrict__ table, int b, long long staging_bytes, long long rows)
{
    const int64_t *r = table + (size_t)b * PLY_DEV_ROW;
    PlyCloud c;
    c.src = r[0], c.stride = r[1], c.big = r[8] != 0, c.n = r[9], c.dst = r[10], c.cap = r[11];
    bool ok = c.src >= 0 && c.src <= staging_bytes && c.stride >= 1 && c.stride <= PLY_MAX_STRIDE;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        const long long off = r[2 + f], type = r[5 + f];
        const bool fits = type >= 0 && type < PLY_NTYPES && off >= 0 && off + ply_size_of((int)(type & 7)) <= c.stride;
        ok = ok && fits;
        c.off[f] = fits ? (int)off : 0, c.type[f] = fits ? (int)type : PLY_U1;
    }
    if (c.dst < 0 || c.dst > rows) c.dst = 0, c.cap = 0;
    c.cap = min(max(c.cap, 0ll), rows - c.dst);
    c.n = ok ? min(max(c.n, 0ll), min(c.cap, (staging_bytes - c.src) / c.stride)) : 0;
    if (!ok) c.src = 0, c.stride = 1;
    return c;
}

// the bits of one field (lo: its first four bytes in file order, hi: the next four of a float64) -> the bits of its float32
__device__ __forceinline__ unsigned ply_convert(unsigned lo, unsigned hi, int type, bool big)
{
    if (big) {
        if (type == PLY_F8) {
            const unsigned t = __builtin_bswap32(lo);
            lo = __builtin_bswap32(hi), hi = t;
        } else if (type >= PLY_I4) {
            lo = __builtin_bswap32(lo);
        } else if (type >= PLY_I2) {
            lo = ((lo & 0xFFu) << 8) | ((lo >> 8) & 0xFFu);
        }
    }
    switch (type) {
    case PLY_I1: return __float_as_uint((float)(int)(signed char)(lo & 0xFFu));
    case PLY_U1: return __float_as_uint((float)(lo & 0xFFu));
    case PLY_I2: return __float_as_uint((float)(int)(short)(lo & 0xFFFFu));
    case PLY_U2: return __float_as_uint((float)(lo & 0xFFFFu));
    case PLY_I4: return __float_as_uint((float)(int)lo);
    case PLY_U4: return __float_as_uint((float)lo);
    case PLY_F4: return lo;
    default: return __float_as_uint((float)__longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)));
    }
}

// a field that starts at byte p of the staged span, from aligned LDS words
__device__ __forceinline__ unsigned ply_field_lds(const unsigned *__restrict__ w, unsigned p, int type, bool big)
{
    const unsigned i = p >> 2, sh = (p & 3u) * 8u;
    const unsigned w0 = w[i], w1 = w[i + 1];
    const unsigned lo = __builtin_amdgcn_alignbit(w1, w0, sh);
    unsigned hi = 0;
    if (type == PLY_F8) hi = __builtin_amdgcn_alignbit(w[i + 2], w1, sh);
    return ply_convert(lo, hi, type, big);
}

// the same field from single-byte global loads (records longer than PLY_STAGE_STRIDE)
__device__ __forceinline__ unsigned ply_field_bytes(const uint8_t *__restrict__ p, int type, bool big)
{
    const int size = ply_size_of(type);
    unsigned lo = 0, hi = 0;
    for (int j = 0; j < size; ++j) {
        const unsigned v = p[j];
        if (j < 4) lo |= v << (8 * j);
        else hi |= v << (8 * (j - 4));
    }
    return ply_convert(lo, hi, type, big);
}

__global__ __launch_bounds__(PLY_THREADS) void ply_unpack_kernel(const uint8_t *__restrict__ staging, long long staging_bytes,
                                                                 const int64_t *__restrict__ table, const int32_t *__restrict__ tile_prefix, int B,
                                                                 unsigned *__restrict__ out, long long rows)
{
    __shared__ uint4 span[PLY_LDS_QUADS];
    __shared__ unsigned rowsw[3 * PLY_THREADS];
    const int tile = blockIdx.x;
    // the cloud whose tiles hold this one: the last b with tile_prefix[b] <= tile (workgroup-uniform)
    if (tile < tile_prefix[0] || tile >= tile_prefix[B]) return;
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_prefix[mid] <= tile) lo = mid;
        else hi = mid - 1;
    }
    const PlyCloud c = ply_cloud(table, lo, staging_bytes, rows);
    const long long row0 = (long long)(tile - tile_prefix[lo]) * PLY_THREADS;
    if (row0 >= c.cap) return;                                          // nothing to do: left before any barrier
    const int live = (int)min((long long)PLY_THREADS, c.cap - row0);    // rows of this tile inside the cloud's capacity
    const int cnt = (int)min(max(c.n - row0, 0ll), (long long)live);    // ... of which records
    const int t = threadIdx.x;
    unsigned v[3] = {0x7FC00000u, 0x7FC00000u, 0x7FC00000u};
    const long long a = c.src + row0 * c.stride;                        // first byte of the tile's span (only used when cnt > 0)
    if (c.stride <= PLY_STAGE_STRIDE) {
        if (cnt > 0) {
            const long long a0 = a & ~15ll;
            const int quads = (int)((a + (long long)cnt * c.stride - a0 + 15) >> 4);    // <= PLY_LDS_QUADS - 1; ends inside staging_bytes (a multiple of 16)
            const uint4 *g = (const uint4 *)(staging + a0);
            for (int q = t; q < quads; q += PLY_THREADS) span[q] = g[q];
        }
        __syncthreads();                                                // cnt is workgroup-uniform, and so is this barrier
        if (t < cnt) {
            const unsigned p = (unsigned)(a & 15ll) + (unsigned)t * (unsigned)c.stride;
#pragma unroll
            for (int f = 0; f < 3; ++f) v[f] = ply_field_lds((const unsigned *)span, p + (unsigned)c.off[f], c.type[f], c.big);
        }
    } else if (t < cnt) {
        const uint8_t *p = staging + a + (long long)t * c.stride;
#pragma unroll
        for (int f = 0; f < 3; ++f) v[f] = ply_field_bytes(p + c.off[f], c.type[f], c.big);
    }
    // the tile's rows are 3 * live consecutive words of out: through LDS, so that a wave stores 64 consecutive words per instruction
    // instead of three words per lane 12 bytes apart (words 3t .. 3t+2 of the lanes fall on different banks: 3 is odd)
    rowsw[3 * t] = v[0], rowsw[3 * t + 1] = v[1], rowsw[3 * t + 2] = v[2];
    __syncthreads();                                                    // every thread that is still here reaches it
    unsigned *o = out + 3 * (size_t)(c.dst + row0);
    for (int i = t; i < 3 * live; i += PLY_THREADS) o[i] = rowsw[i];
}

}  // namespace

extern "C" int pccx_ply_unpack(const void *staging, int64_t staging_bytes, const int64_t *table, const int32_t *tile_prefix, int B,
                               int64_t total_tiles, float *out, int64_t rows, void *stream)
{
    PCCX_CHECK_ARG(B >= 0 && total_tiles >= 0 && rows >= 0 && staging_bytes >= 0, "pccx_ply_unpack: negative size");
    PCCX_CHECK_ARG(total_tiles <= 2147483647ll, "pccx_ply_unpack: %lld tiles of 256 rows, at most 2^31 - 1 per call", (long long)total_tiles);
    if (B == 0 || total_tiles == 0) return PCCX_OK;
    PCCX_CHECK_ARG(staging && table && tile_prefix && out, "pccx_ply_unpack: null pointer");
    PCCX_CHECK_ARG((uintptr_t)staging % 16 == 0 && staging_bytes % 16 == 0,
                   "pccx_ply_unpack: the staging buffer must start at a multiple of 16 bytes and be a multiple of 16 bytes long (it is read by 16-byte loads)");
    hipLaunchKernelGGL(ply_unpack_kernel, dim3((unsigned)total_tiles), dim3(PLY_THREADS), 0, (hipStream_t)stream, (const uint8_t *)staging,
                       (long long)staging_bytes, table, tile_prefix, B, (unsigned *)out, (long long)rows);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}
