// rangecoder.hip -- torchac-style range coder (compress.py:136 encode_float_cdf, decompress.py:93
// decode_float_cdf) on the GPU: 32-bit low/high, 16-bit CDFs, E1/E2/E3 renormalisation with pending
// bits, MSB-first bit packing, zero-padded last byte.  Byte layout PARITY UNPINNED (torchac is not in
// the image); the oracle (orc_range_encode / orc_range_decode) restates the same published algorithm
// and must agree byte-for-byte.
//
// The coder is inherently serial per stream (S*d = 1024 symbols per cloud).  One wave per cloud:
// the 64 lanes stage the cloud's tables and bytes through LDS with coalesced transfers and run the
// serial recurrence wave-uniformly on the scalar unit (see "wave-uniform execution" below).  Streams
// larger than the LDS budget fall back to one lane per cloud working from global memory.  The opt-in
// split form (split_stream.h) cuts a cloud's stream into segments that each fit the budget, one wave
// per segment.
#include "common.h"
#include "split_stream.h"
#include "entry_index.h"

struct BitWriter {
    uint8_t *buf;
    int cap, n;
    unsigned cache;
    int count;
    __device__ void bit(int b)
    {
        cache = (cache << 1) | (unsigned)(b & 1);
        if (++count == 8) {
            if (n < cap) buf[n] = (uint8_t)cache;
            ++n;
            count = 0; cache = 0;
        }
    }
    __device__ void bit_pending(int b, unsigned long long &pending)
    {
        bit(b);
        while (pending > 0) { bit(!b); --pending; }
    }
    __device__ void flush()
    {
        if (count > 0) {
            cache <<= (8 - count);
            if (n < cap) buf[n] = (uint8_t)cache;
            ++n;
            count = 0; cache = 0;
        }
    }
};

// A row's byte count as the decoders take it: cut to the row before anything is read; the encoder's overflow mark (negative) reads as 0.
__device__ __forceinline__ int rc_row_bytes(int count, int stride) { return count < 0 ? 0 : (count > stride ? stride : count); }

// The entry of the index (entry_index.h) a coder is at: its interval, the bits behind it (emitted plus pending on the encoder,
// shifted in beyond the first 32 on the decoder -- the same number) and whether an underflow run is pending.  One 12-byte store.
// Outside the coder's contract -- a table with a zero-width symbol can drive high below low (see `fix` in rc_encode_wave) -- the state
// is recorded as it is; such an entry fails pccx_index_state_ok, so the indexed decoder refuses that cloud's sidecar with status 6
// where the sequential decoder returns symbols (which are not the coded ones either: such a stream does not decode to its input).
__device__ __forceinline__ void rc_record(uint32_t *entry, unsigned low, unsigned high, unsigned long long bits, bool pending)
{
    entry[0] = low;
    entry[1] = high;
    entry[2] = (unsigned)(bits < 0x7FFFFFFFull ? bits : 0x7FFFFFFFull) | (pending ? PCCX_INDEX_FLAG : 0u);
}
// The 16 fixed bytes of a sidecar at `index` (4-byte aligned).
__device__ __forceinline__ void rc_index_header(uint32_t *index, int nsym, int seg_sym)
{
    index[0] = 0x31495850u;                                            // "PXI1", little-endian
    index[1] = (unsigned)nsym;
    index[2] = (unsigned)seg_sym;
    index[3] = (unsigned)pccx_index_segments(nsym, seg_sym);
}

// One lane per cloud.  REC: also write the cloud's sidecar of idx_stride bytes at index + b * idx_stride (the header and the entry at
// every seg_sym boundary); the stream does not depend on it.
// nsym_of (ragged batches; null otherwise): the rows of cdf_int / latent_q are nsym symbols apart and cloud b codes its first nsym_of[b].
template <bool REC>
__device__ __forceinline__ void rc_encode_lane(const int32_t *__restrict__ cdf_int, const float *__restrict__ latent_q, int B, int nsym,
                                               int Lp, int sym_offset, uint8_t *__restrict__ out, int cap, int32_t *__restrict__ nbytes,
                                               int seg_sym, uint8_t *__restrict__ index, int idx_stride,
                                               const int32_t *__restrict__ nsym_of = nullptr)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int row = nsym;
    if (nsym_of) nsym = rc_row_bytes(nsym_of[b], row);
    uint32_t *entry = nullptr;
    if (REC) {
        entry = (uint32_t *)(index + (size_t)b * idx_stride);
        rc_index_header(entry, nsym, seg_sym);
        entry += PCCX_INDEX_HEADER_BYTES / 4;
    }
    BitWriter w{out + (size_t)b * cap, cap, 0, 0u, 0};
    unsigned low = 0u, high = 0xFFFFFFFFu;
    unsigned long long pending = 0;
    const int max_symbol = Lp - 2;
    const int32_t *c = cdf_int + (size_t)b * row * Lp;
    const float *q = latent_q + (size_t)b * row;
    // Without REC one pass over all symbols; with it one pass per segment (seg_sym >= 1: P passes), the entry stored in front of
    // each, so that the symbol loop itself carries no test for a boundary.
    int i = 0, stop = REC ? 0 : nsym;
    do {
    if (REC && i < nsym) {
        rc_record(entry, low, high, (unsigned long long)w.n * 8ull + (unsigned long long)w.count + pending, pending > 0);
        entry += PCCX_INDEX_ENTRY_BYTES / 4;
        stop = nsym - i < seg_sym ? nsym : i + seg_sym;
    }
    for (; i < stop; ++i, c += Lp) {
        int s = (int)q[i] + sym_offset;                       // latent_quantized.to(int16) + L//2 (compress.py:135)
        s = s < 0 ? 0 : (s > max_symbol ? max_symbol : s);
        const unsigned long long span = (unsigned long long)high - (unsigned long long)low + 1ull;
        const unsigned c_low = (unsigned)c[s] & 0xFFFFu;
        const unsigned c_high = s == max_symbol ? 0x10000u : ((unsigned)c[s + 1] & 0xFFFFu);
        high = (unsigned)((low - 1u) + (unsigned)((span * c_high) >> 16));
        low = (unsigned)(low + (unsigned)((span * c_low) >> 16));
        for (;;) {
            if (high < 0x80000000u) {
                w.bit_pending(0, pending);
                low <<= 1; high <<= 1; high |= 1u;
            } else if (low >= 0x80000000u) {
                w.bit_pending(1, pending);
                low <<= 1; high <<= 1; high |= 1u;
            } else if (low >= 0x40000000u && high < 0xC0000000u) {
                ++pending;
                low <<= 1; low &= 0x7FFFFFFFu;
                high <<= 1; high |= 0x80000001u;
            } else
                break;
        }
    }
    } while (REC && i < nsym);
    ++pending;
    if (low < 0x40000000u) w.bit_pending(0, pending);
    else w.bit_pending(1, pending);
    w.flush();
    nbytes[b] = w.n <= cap ? w.n : -w.n;                      // negative: capacity exceeded
}

__global__ void range_encode_kernel(const int32_t *__restrict__ cdf_int, const float *__restrict__ latent_q, int B, int nsym,
                                    int Lp, int sym_offset, uint8_t *__restrict__ out, int cap, int32_t *__restrict__ nbytes)
{
    rc_encode_lane<false>(cdf_int, latent_q, B, nsym, Lp, sym_offset, out, cap, nbytes, 0, nullptr, 0);
}

__global__ void range_encode_indexed_kernel(const int32_t *__restrict__ cdf_int, const float *__restrict__ latent_q, int B, int nsym,
                                            int Lp, int sym_offset, uint8_t *__restrict__ out, int cap, int32_t *__restrict__ nbytes,
                                            int seg_sym, uint8_t *__restrict__ index, int idx_stride)
{
    rc_encode_lane<true>(cdf_int, latent_q, B, nsym, Lp, sym_offset, out, cap, nbytes, seg_sym, index, idx_stride);
}

// One lane per cloud.  REC: write the cloud's sidecar as rc_encode_lane does (the decoder passes through the encoder's states), and
// latent_q may then be null.
// nsym_of: as rc_encode_lane; the latents of cloud b from nsym_of[b] on are written as zeros.
template <bool REC>
__device__ __forceinline__ void rc_decode_lane(const int32_t *__restrict__ cdf_int, const uint8_t *__restrict__ in, int stride,
                                               const int32_t *__restrict__ nbytes, int B, int nsym, int Lp, int sym_offset,
                                               float *__restrict__ latent_q, int seg_sym, uint8_t *__restrict__ index, int idx_stride,
                                               const int32_t *__restrict__ nsym_of = nullptr)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int row = nsym;
    if (nsym_of) {
        nsym = rc_row_bytes(nsym_of[b], row);
        for (int i = nsym; i < row; ++i) latent_q[(size_t)b * row + i] = 0.f;
    }
    uint32_t *entry = nullptr;
    int next = 0;
    unsigned long long shifted = 0;                           // REC: bits taken beyond the first 32; an underflow run is pending
    bool under = false;
    if (REC) {
        entry = (uint32_t *)(index + (size_t)b * idx_stride);
        rc_index_header(entry, nsym, seg_sym);
        entry += PCCX_INDEX_HEADER_BYTES / 4;
    }
    const uint8_t *buf = in + (size_t)b * stride;
    const int nb = rc_row_bytes(nbytes[b], stride);
    int pos = 0, cached = 0;
    unsigned cache = 0;
    unsigned low = 0u, high = 0xFFFFFFFFu, value = 0u;
    auto get = [&]() {
        if (cached == 0) {
            if (pos >= nb) { value <<= 1; return; }
            cache = buf[pos++]; cached = 8;
        }
        value = (value << 1) | ((cache >> (cached - 1)) & 1u);
        --cached;
    };
    for (int i = 0; i < 32; ++i) get();
    const int max_symbol = Lp - 2;
    const int32_t *c = cdf_int + (size_t)b * row * Lp;
    for (int i = 0; i < nsym; ++i, c += Lp) {
        if (REC && i == next) {
            rc_record(entry, low, high, shifted, under);
            entry += PCCX_INDEX_ENTRY_BYTES / 4;
            next += seg_sym;
        }
        const unsigned long long span = (unsigned long long)high - (unsigned long long)low + 1ull;
        const unsigned count =
            (unsigned)((((unsigned long long)value - (unsigned long long)low + 1ull) * 0x10000ull - 1ull) / span) & 0xFFFFu;
        int left = 0, right = max_symbol + 1;
        while (left + 1 < right) {
            const int mid = (left + right) >> 1;
            if (((unsigned)c[mid] & 0xFFFFu) <= count) left = mid; else right = mid;
        }
        const int s = left;
        if (!REC || latent_q) latent_q[(size_t)b * row + i] = (float)(s - sym_offset);            // decode - L//2 (decompress.py:93)
        const unsigned c_low = (unsigned)c[s] & 0xFFFFu;
        const unsigned c_high = s == max_symbol ? 0x10000u : ((unsigned)c[s + 1] & 0xFFFFu);
        high = (unsigned)((low - 1u) + (unsigned)((span * c_high) >> 16));
        low = (unsigned)(low + (unsigned)((span * c_low) >> 16));
        for (;;) {
            if (low >= 0x80000000u || high < 0x80000000u) {
                low <<= 1; high <<= 1; high |= 1u; get();
                if (REC) ++shifted, under = false;
            } else if (low >= 0x40000000u && high < 0xC0000000u) {
                low <<= 1; low &= 0x7FFFFFFFu;
                high <<= 1; high |= 0x80000001u;
                value -= 0x40000000u;
                get();
                if (REC) ++shifted, under = true;
            } else
                break;
        }
    }
}

__global__ void range_decode_kernel(const int32_t *__restrict__ cdf_int, const uint8_t *__restrict__ in, int stride,
                                    const int32_t *__restrict__ nbytes, int B, int nsym, int Lp, int sym_offset,
                                    float *__restrict__ latent_q)
{
    rc_decode_lane<false>(cdf_int, in, stride, nbytes, B, nsym, Lp, sym_offset, latent_q, 0, nullptr, 0);
}

__global__ void range_index_build_kernel(const int32_t *__restrict__ cdf_int, const uint8_t *__restrict__ in, int stride,
                                         const int32_t *__restrict__ nbytes, int B, int nsym, int Lp, int sym_offset,
                                         float *__restrict__ latent_q, int seg_sym, uint8_t *__restrict__ index, int idx_stride)
{
    rc_decode_lane<true>(cdf_int, in, stride, nbytes, B, nsym, Lp, sym_offset, latent_q, seg_sym, index, idx_stride);
}

__global__ void range_encode_n_kernel(const int32_t *__restrict__ cdf_int, const float *__restrict__ latent_q, int B, int row,
                                      const int32_t *__restrict__ nsym_of, int Lp, int sym_offset, uint8_t *__restrict__ out, int cap,
                                      int32_t *__restrict__ nbytes)
{
    rc_encode_lane<false>(cdf_int, latent_q, B, row, Lp, sym_offset, out, cap, nbytes, 0, nullptr, 0, nsym_of);
}

__global__ void range_decode_n_kernel(const int32_t *__restrict__ cdf_int, const uint8_t *__restrict__ in, int stride,
                                      const int32_t *__restrict__ nbytes, int B, int row, const int32_t *__restrict__ nsym_of, int Lp,
                                      int sym_offset, float *__restrict__ latent_q)
{
    rc_decode_lane<false>(cdf_int, in, stride, nbytes, B, row, Lp, sym_offset, latent_q, 0, nullptr, 0, nsym_of);
}

#define RC_MAX_LDS_BYTES (60 * 1024)

// ---- bulk renormalisation -----------------------------------------------------------------------
// The E1/E2 loop of the reference coder shifts out one bit per iteration while the top bits of low
// and high agree; that run is clz(low ^ high) bits long and can be emitted at once.  The E3
// (underflow) loop runs while low = 01.., high = 10..: its length is the run of positions, from bit
// 30 down, where low has 1 and high has 0, again one clz.  k consecutive E3 steps give
//   low' = (low << k) & 0x7FFFFFFF,  high' = (high << k) | 0x80000000 | (2^k - 1),  pending += k,
// and on the decoder value' = ((value << k) ^ 0x80000000) | next k bits (each step subtracts 2^30
// before doubling; the k subtractions sum to 2^31 mod 2^32).  Bit-for-bit the same stream as the
// one-bit-at-a-time form (tests compare against the oracle's literal restatement).
// Loop shape: after an E1/E2 run the top bits of low and high differ (0 / 1), an E3 run keeps them so, and
// after an E3 run the E3 condition is false by construction, so the renormalisation "loop" is exactly one
// optional E1/E2 run followed by one optional E3 run; with t = (~low | high) << 1 the E3 run length is
// clz(t) (0 when there is no underflow, because then bit 31 of t is set), which makes both steps branch-free.
// ---- wave-uniform execution -------------------------------------------------------------------
// The recurrence (low, high, value, pending, the bit accumulators) lives in SCALAR registers: every
// quantity below that does not depend on the lane is derived from readlane / ballot / readfirstlane,
// so the compiler keeps it on the SALU (s_mul_hi_u32, s_flbit, s_lshl_b64 ...) and no step of the serial
// chain waits on an LDS or memory round trip:
//   encoder  a parallel pre-pass gathers (cdf[s], cdf[s+1]) of every symbol into LDS; the serial loop
//            takes them 64 symbols at a time into one VGPR pair (next block prefetched) and reads
//            symbol j with v_readlane.  Output bits go through a 64-bit scalar accumulator and leave
//            as whole big-endian words.
//   decoder  the 64 lanes hold the CDF rows of G = 64 / (L+1) consecutive symbols (next block
//            prefetched from LDS).  Per symbol ALL candidates are scaled at once
//            (t = ((span * cdf) >> 16), one v_mad_u64_u32 + shift per lane), compared with value - low,
//            and the ballot mask is walked with the reference's binary search, on scalar bits; the
//            two t's that become the new low/high come back with v_readlane.  Input bits are taken
//            from a 64-bit scalar buffer refilled a word at a time, the next word always already
//            loaded.
__device__ __forceinline__ unsigned ones(int m) { return m >= 32 ? 0xFFFFFFFFu : ((1u << m) - 1u); }
__device__ __forceinline__ unsigned rc_uni(unsigned v) { return __builtin_amdgcn_readfirstlane(v); }
// low 32 bits of (span * c) >> 16 with span = span32 + 1 in [1, 2^32]
__device__ __forceinline__ unsigned rc_scale(unsigned span32, unsigned c) { return (unsigned)(((unsigned long long)span32 * c + c) >> 16); }

// One stream, one wave: c = the stream's tables [nsym][Lp], q = its nsym latents, out = its cap bytes, nbytes = its count.  The
// pointers and counts must be wave-uniform (kernel arguments and blockIdx only).  LDS: rc_encode_lds(nsym, cap) bytes at smem.
// REC: lane 0 also stores the entry (rc_record) of every seg_sym boundary at entry, entry + 3, ...; the stream does not depend on it,
// and without REC the two arguments are not looked at.
template <bool REC = false>
__device__ __forceinline__ void rc_encode_wave(unsigned char *smem, const int32_t *__restrict__ c, const float *__restrict__ q, int nsym,
                                               int Lp, int sym_offset, uint8_t *__restrict__ out, int cap, int32_t *__restrict__ nbytes,
                                               uint32_t *__restrict__ entry = nullptr, int seg_sym = 0)
{
    uint2 *sc = (uint2 *)smem;                                         // [nsym] (c_low, c_high)
    unsigned *sout = (unsigned *)(sc + nsym);                          // [capw] output words (stream order = big endian)
    const int lane = threadIdx.x;
    const int capw = (cap + 3) >> 2;
    const int max_symbol = Lp - 2;
    for (int i = lane; i < nsym; i += 64) {
        int s = (int)q[i] + sym_offset;                               // latent_quantized.to(int16) + L//2 (compress.py:135)
        s = s < 0 ? 0 : (s > max_symbol ? max_symbol : s);
        const int32_t *ci = c + (size_t)i * Lp;
        sc[i] = make_uint2((unsigned)ci[s] & 0xFFFFu, s == max_symbol ? 0x10000u : ((unsigned)ci[s + 1] & 0xFFFFu));
    }
    __syncthreads();
    unsigned low = 0u, high = 0xFFFFFFFFu;
    unsigned long long pending = 0, acc = 0;
    int na = 0, nw = 0;
    auto put = [&](unsigned v, int cnt) {                              // cnt <= 32; na < 32 on entry
        acc = (acc << cnt) | (unsigned long long)v;
        na += cnt;
        if (na >= 32) {
            const unsigned w = (unsigned)(acc >> (na - 32));
            if (nw < capw && lane == 0) sout[nw] = __builtin_bswap32(w);
            ++nw;
            na -= 32;
        }
    };
    auto run = [&](int bit, unsigned long long cnt) {
        while (cnt > 0) {
            const int m = cnt > 32 ? 32 : (int)cnt;
            put(bit ? ones(m) : 0u, m);
            cnt -= m;
        }
    };
    int next = 0;                                                      // REC: the next boundary
    uint2 nxt = lane < nsym ? sc[lane] : make_uint2(0u, 0x10000u);
    for (int i0 = 0; i0 < nsym; i0 += 64) {
        const uint2 cur = nxt;
        if (i0 + 64 + lane < nsym) nxt = sc[i0 + 64 + lane];
        const int cnt = nsym - i0 < 64 ? nsym - i0 : 64;
        for (int j = 0; j < cnt; ++j) {
            if (REC && i0 + j == next) {
                if (lane == 0) rc_record(entry, low, high, (unsigned long long)nw * 32ull + (unsigned long long)na + pending, pending > 0);
                entry += PCCX_INDEX_ENTRY_BYTES / 4;
                next += seg_sym;
            }
            const unsigned c_low = __builtin_amdgcn_readlane(cur.x, j), c_high = __builtin_amdgcn_readlane(cur.y, j);
            const unsigned span32 = high - low;
            high = (low - 1u) + rc_scale(span32, c_high);
            low = low + rc_scale(span32, c_low);
            // Renormalisation, branch-free (see "loop shape" above): one E1/E2 run of m bits, then one E3 run of k.
            const unsigned x = low ^ high;
            const int m = (int)x < 0 ? 0 : (x ? __clz(x) : 32);
            if (m > 0) {
                const unsigned top = (unsigned)(((unsigned long long)low << m) >> 32);     // the m agreeing bits
                if (pending == 0)
                    put(top, m);
                else {
                    const unsigned b0 = low >> 31;
                    put(b0, 1);
                    run(!b0, pending);
                    pending = 0;
                    if (m > 1) put(top & ones(m - 1), m - 1);
                }
                low = (unsigned)((unsigned long long)low << m);
                high = (unsigned)(((unsigned long long)high << m) | (unsigned long long)ones(m));
            }
            const unsigned t = (~low | high) << 1;                       // top bit set <=> no underflow pending
            const int k = t ? __clz(t) : 31;
            const unsigned fix = k ? 0x80000000u : 0u;                  // k = 0 must leave low/high alone (also when a zero-width
            low = (low << k) & ~fix;                                     // symbol has driven high below low)
            high = (high << k) | fix | ones(k);
            pending += k;
        }
    }
    ++pending;
    const int fb = low < 0x40000000u ? 0 : 1;
    put(fb, 1);
    run(!fb, pending);
    int n = nw * 4 + ((na + 7) >> 3);
    if (na > 0 && nw < capw && lane == 0) sout[nw] = __builtin_bswap32((unsigned)(acc << (32 - na)));   // zero-padded tail
    if (lane == 0) *nbytes = n <= cap ? n : -n;                        // negative: capacity exceeded
    __syncthreads();
    if (n > cap) n = cap;
    const uint8_t *sb = (const uint8_t *)sout;
    for (int i = lane; i < n; i += 64) out[i] = sb[i];
}

__global__ __launch_bounds__(64) void range_encode_wave_kernel(const int32_t *__restrict__ cdf_int, const float *__restrict__ latent_q,
                                                               int nsym, int Lp, int sym_offset, uint8_t *__restrict__ out, int cap,
                                                               int32_t *__restrict__ nbytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
    const int b = blockIdx.x;
    rc_encode_wave(rc_smem, cdf_int + (size_t)b * nsym * Lp, latent_q + (size_t)b * nsym, nsym, Lp, sym_offset, out + (size_t)b * cap, cap,
                   nbytes + b);
}

// Ragged batch, one wave per cloud: rows of `row` symbols, of which cloud b codes its first nsym_of[b] (LDS sized for the row).
__global__ __launch_bounds__(64) void range_encode_wave_n_kernel(const int32_t *__restrict__ cdf_int, const float *__restrict__ latent_q,
                                                                 int row, const int32_t *__restrict__ nsym_of, int Lp, int sym_offset,
                                                                 uint8_t *__restrict__ out, int cap, int32_t *__restrict__ nbytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
    const int b = blockIdx.x;
    rc_encode_wave(rc_smem, cdf_int + (size_t)b * row * Lp, latent_q + (size_t)b * row, rc_row_bytes(nsym_of[b], row), Lp, sym_offset,
                   out + (size_t)b * cap, cap, nbytes + b);
}

// One stream, one wave: c = the stream's tables [nsym][Lp], in = its first byte, nb = its length already clamped to [0, stride]
// (bytes from nb on are not read and count as zero), q = its nsym outputs.  The pointers and counts must be wave-uniform.  LDS:
// rc_decode_lds(nsym, Lp - 1, stride) bytes at smem.
// INIT: the stream is entered at an entry of its index (entry_index.h): `in` is the byte that holds stream bit pos, skip = pos & 7
// the bits of it that lie before pos, (low0, high0) the interval and under0 the pending flag; value is rebuilt from the 32 bits at pos.
// REC: lane 0 also stores the entry of every seg_sym boundary at entry, entry + 3, ... (rc_record), and q may be null.
// Without INIT / REC their arguments are not looked at.
template <bool INIT = false, bool REC = false>
__device__ __forceinline__ void rc_decode_wave(unsigned char *smem, const int32_t *__restrict__ c, const uint8_t *__restrict__ in, int stride,
                                               int nb, int nsym, int Lp, int sym_offset, float *__restrict__ q, unsigned low0 = 0u,
                                               unsigned high0 = 0xFFFFFFFFu, int skip = 0, bool under0 = false,
                                               uint32_t *__restrict__ entry = nullptr, int seg_sym = 0)
{
    const int ncdf = nsym * Lp;
    unsigned short *scdf = (unsigned short *)smem;                    // [ncdf]
    unsigned *sin = (unsigned *)(smem + (((size_t)ncdf * 2 + 3) & ~(size_t)3));      // [nwin] stream words, zero padded
    unsigned char *ssym = (unsigned char *)(sin + ((stride + 3) >> 2));               // [nsym]
    const int lane = threadIdx.x;
    const int nwin = (nb + 3) >> 2;
    for (int i = lane; i < ncdf; i += 64) scdf[i] = (unsigned short)c[i];
    for (int i = lane; i < nwin * 4; i += 64) ((uint8_t *)sin)[i] = i < nb ? in[i] : (uint8_t)0;
    __syncthreads();
    // bit reader: `buf` holds `have` unread bits in its low end, `nxt` is the word after them; words past
    // the stream read as 0
    auto word = [&](int p) -> unsigned { return p < nwin ? __builtin_bswap32(rc_uni(sin[p])) : 0u; };
    unsigned long long buf = 0;
    int have = 0, pos = 1;
    unsigned nxt = word(0);
    auto getbits = [&](int m) -> unsigned {                            // m <= 32
        if (have < m) {
            buf = (buf << 32) | (unsigned long long)nxt;
            have += 32;
            nxt = word(pos);
            ++pos;
        }
        have -= m;
        return (unsigned)(buf >> have) & ones(m);
    };
    unsigned low = 0u, high = 0xFFFFFFFFu;
    if (INIT) {
        low = low0, high = high0;
        getbits(skip & 7);
    }
    unsigned value = getbits(32);
    if (INIT) value ^= under0 ? 0x80000000u : 0u;
    unsigned long long shifted = 0;                                    // REC: bits taken beyond the first 32; an underflow run is pending
    bool under = false;
    int next = 0;
    const int max_symbol = Lp - 2;
    const int G = 64 / Lp;                                             // symbols per block of lanes
    unsigned cn = lane < G * Lp && lane < ncdf ? scdf[lane] : 0u;
    for (int i0 = 0; i0 < nsym; i0 += G) {
        const unsigned cv = cn;
        const int inext = (i0 + G) * Lp + lane;
        if (lane < G * Lp && inext < ncdf) cn = scdf[inext];
        const int cnt = nsym - i0 < G ? nsym - i0 : G;
        for (int j = 0; j < cnt; ++j) {
            if (REC && i0 + j == next) {
                if (lane == 0) rc_record(entry, low, high, shifted, under);
                entry += PCCX_INDEX_ENTRY_BYTES / 4;
                next += seg_sym;
            }
            const unsigned span32 = high - low, off = value - low;
            // largest s with cdf[s] <= ((value-low+1)*2^16 - 1) / span  <=>  (span*cdf[s]) >> 16 <= value - low
            const unsigned t = rc_scale(span32, cv);
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(t <= off) >> (j * Lp);
            // A monotone table gives a run of ones from bit 1 up and the search result is its length; any other
            // pattern walks the reference's binary search literally.
            const unsigned long long mr = (mask >> 1) & (~0ull >> (64 - max_symbol));
            int s = __popcll(mr);
            if ((mr + 1ull) & mr) {
                int left = 0, right = max_symbol + 1;
                while (left + 1 < right) {
                    const int mid = (left + right) >> 1;
                    if ((mask >> mid) & 1ull) left = mid; else right = mid;
                }
                s = left;
            }
            if (lane == 0) ssym[i0 + j] = (unsigned char)s;
            const unsigned t_low = __builtin_amdgcn_readlane(t, j * Lp + s);
            if (s != max_symbol) high = (low - 1u) + __builtin_amdgcn_readlane(t, j * Lp + s + 1);   // c_high = 2^16 leaves high as is
            low = low + t_low;
            const unsigned x = low ^ high;
            const int m = (int)x < 0 ? 0 : (x ? __clz(x) : 32);
            low = (unsigned)((unsigned long long)low << m);
            high = (unsigned)(((unsigned long long)high << m) | (unsigned long long)ones(m));
            const unsigned tt = (~low | high) << 1;
            const int k = tt ? __clz(tt) : 31;
            const unsigned fix = k ? 0x80000000u : 0u;
            low = (low << k) & ~fix;
            high = (high << k) | fix | ones(k);
            // value' = ((value << m | bits_m) << k ^ 2^31) | bits_k  =  (value << (m+k) | bits_(m+k)) ^ (k ? 2^31 : 0)
            const int n = m + k;
            if (REC) shifted += (unsigned)n, under = k > 0 || (m == 0 && under);
            if (n <= 32) {
                const unsigned nbits = getbits(n);
                value = ((unsigned)((unsigned long long)value << n) | nbits) ^ fix;
            } else {                                                   // a long E1/E2 run followed by a long E3 run (m, k <= 31)
                const unsigned v1 = (value << m) | getbits(m);
                value = ((v1 << k) ^ 0x80000000u) | getbits(k);
            }
        }
    }
    __syncthreads();
    if (REC && !q) return;
    for (int i = lane; i < nsym; i += 64) q[i] = (float)((int)ssym[i] - sym_offset);
}

__global__ __launch_bounds__(64) void range_decode_wave_kernel(const int32_t *__restrict__ cdf_int, const uint8_t *__restrict__ in,
                                                               int stride, const int32_t *__restrict__ nbytes, int nsym, int Lp,
                                                               int sym_offset, float *__restrict__ latent_q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
    const int b = blockIdx.x;
    const int nb = rc_row_bytes(nbytes[b], stride);
    rc_decode_wave(rc_smem, cdf_int + (size_t)b * nsym * Lp, in + (size_t)b * stride, stride, nb, nsym, Lp, sym_offset,
                   latent_q + (size_t)b * nsym);
}

// Ragged batch: as range_encode_wave_n_kernel; the latents from nsym_of[b] on are written as zeros.
__global__ __launch_bounds__(64) void range_decode_wave_n_kernel(const int32_t *__restrict__ cdf_int, const uint8_t *__restrict__ in,
                                                                 int stride, const int32_t *__restrict__ nbytes, int row,
                                                                 const int32_t *__restrict__ nsym_of, int Lp, int sym_offset,
                                                                 float *__restrict__ latent_q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
    const int b = blockIdx.x;
    const int nb = rc_row_bytes(nbytes[b], stride), ns = rc_row_bytes(nsym_of[b], row);
    float *q = latent_q + (size_t)b * row;
    rc_decode_wave(rc_smem, cdf_int + (size_t)b * row * Lp, in + (size_t)b * stride, stride, nb, ns, Lp, sym_offset, q);
    for (int i = ns + threadIdx.x; i < row; i += 64) q[i] = 0.f;
}

// LDS images of the two wave kernels: (c_low, c_high) per symbol + the output words; the 16-bit tables + the stream words +
// one byte per decoded symbol.
static size_t rc_encode_lds(int nsym, int cap) { return (size_t)nsym * 8 + (size_t)((cap + 3) / 4) * 4; }
static size_t rc_decode_lds(int nsym, int L, int stride)
{
    return (((size_t)nsym * (L + 1) * 2 + 3) & ~(size_t)3) + (size_t)((stride + 3) / 4) * 4 + (size_t)nsym;
}

// The one statement of which kernel a call runs: 0 = one wave per cloud (its LDS image fits RC_MAX_LDS_BYTES; the wave decoder also
// needs the L+1 table entries of a symbol on the 64 lanes and a search mask of at least one bit, 2 <= L <= 63), 1 = one lane per cloud.
extern "C" int pccx_range_coder_form(int decode, int nsym, int L, int cap_or_stride)
{
    if (nsym < 0 || L < 1 || cap_or_stride < 0) return 1;
    if (decode) return rc_decode_lds(nsym, L, cap_or_stride) <= RC_MAX_LDS_BYTES && L >= 2 && L + 1 <= 64 ? 0 : 1;
    return rc_encode_lds(nsym, cap_or_stride) <= RC_MAX_LDS_BYTES ? 0 : 1;
}

extern "C" int pccx_range_encode(const int32_t *cdf_int, const float *latent_q, int B, int nsym, int L, uint8_t *out, int cap,
                                 int32_t *nbytes, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    PCCX_CHECK_ARG(cdf_int && latent_q && out && nbytes, "pccx_range_encode: null pointer");
    PCCX_CHECK_ARG(B >= 0 && nsym >= 0 && L >= 1 && cap >= 8, "pccx_range_encode: bad shape");
    const size_t lds = rc_encode_lds(nsym, cap);
    if (pccx_range_coder_form(0, nsym, L, cap) == 0) {
        hipLaunchKernelGGL(range_encode_wave_kernel, dim3(B), dim3(64), lds, (hipStream_t)stream, cdf_int, latent_q, nsym, L + 1,
                           L / 2, out, cap, nbytes);
        PCCX_CHECK_LAUNCH();
        return PCCX_OK;
    }
    hipLaunchKernelGGL(range_encode_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cdf_int, latent_q, B, nsym,
                       L + 1, L / 2, out, cap, nbytes);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

extern "C" int pccx_range_decode(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, int B, int nsym,
                                 int L, float *latent_q, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    PCCX_CHECK_ARG(cdf_int && in && nbytes && latent_q, "pccx_range_decode: null pointer");
    PCCX_CHECK_ARG(B >= 0 && nsym >= 0 && L >= 1 && stride >= 1, "pccx_range_decode: bad shape");
    const size_t lds = rc_decode_lds(nsym, L, stride);
    if (pccx_range_coder_form(1, nsym, L, stride) == 0) {
        hipLaunchKernelGGL(range_decode_wave_kernel, dim3(B), dim3(64), lds, (hipStream_t)stream, cdf_int, in, stride, nbytes, nsym,
                           L + 1, L / 2, latent_q);
        PCCX_CHECK_LAUNCH();
        return PCCX_OK;
    }
    hipLaunchKernelGGL(range_decode_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cdf_int, in, stride, nbytes,
                       B, nsym, L + 1, L / 2, latent_q);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

// Ragged batches: nsym = the row stride of cdf_int / latent_q in symbols, nsym_of[b] <= nsym the symbols cloud b codes from a fresh
// state.  The form is chosen by the row as pccx_range_coder_form does; the bytes are pccx_range_encode's on the same table and symbols.
extern "C" int pccx_range_encode_n(const int32_t *cdf_int, const float *latent_q, int B, int nsym, const int32_t *nsym_of, int L,
                                   uint8_t *out, int cap, int32_t *nbytes, void *stream)
{
    if (B == 0) return PCCX_OK;
    PCCX_CHECK_ARG(cdf_int && latent_q && nsym_of && out && nbytes, "pccx_range_encode_n: null pointer");
    PCCX_CHECK_ARG(B >= 0 && nsym >= 0 && L >= 1 && cap >= 8, "pccx_range_encode_n: bad shape");
    if (pccx_range_coder_form(0, nsym, L, cap) == 0)
        hipLaunchKernelGGL(range_encode_wave_n_kernel, dim3(B), dim3(64), rc_encode_lds(nsym, cap), (hipStream_t)stream, cdf_int, latent_q,
                           nsym, nsym_of, L + 1, L / 2, out, cap, nbytes);
    else
        hipLaunchKernelGGL(range_encode_n_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cdf_int, latent_q, B, nsym,
                           nsym_of, L + 1, L / 2, out, cap, nbytes);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

extern "C" int pccx_range_decode_n(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, int B, int nsym,
                                   const int32_t *nsym_of, int L, float *latent_q, void *stream)
{
    if (B == 0) return PCCX_OK;
    PCCX_CHECK_ARG(cdf_int && in && nbytes && nsym_of && latent_q, "pccx_range_decode_n: null pointer");
    PCCX_CHECK_ARG(B >= 0 && nsym >= 0 && L >= 1 && stride >= 1, "pccx_range_decode_n: bad shape");
    if (pccx_range_coder_form(1, nsym, L, stride) == 0)
        hipLaunchKernelGGL(range_decode_wave_n_kernel, dim3(B), dim3(64), rc_decode_lds(nsym, L, stride), (hipStream_t)stream, cdf_int, in,
                           stride, nbytes, nsym, nsym_of, L + 1, L / 2, latent_q);
    else
        hipLaunchKernelGGL(range_decode_n_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cdf_int, in, stride, nbytes, B,
                           nsym, nsym_of, L + 1, L / 2, latent_q);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

// ---- split stream: P independent segments per cloud, one wave each -----------------------------------------------------------
// Layout and header rules: split_stream.h.  Encode = every segment by rc_encode_wave into a scratch row of segcap bytes, then one
// pack kernel per call; decode = one check kernel per call (status + segment offsets per cloud), then every segment by
// rc_decode_wave at its offset.  Scratch: counts (B*P) int32 | rows (B*P, segcap) u8 for encode, offsets (B, P+1) int32 for decode.
static int rc_split_segcap(int seg_sym) { return 2 * seg_sym + 16; }            // models.range_cap

// Largest seg_sym whose LDS images (encode and decode, at segcap bytes per segment) fit RC_MAX_LDS_BYTES; 0 for an L the wave decoder
// does not take.  Both images grow with seg_sym.
extern "C" int pccx_range_split_max_seg_sym(int L)
{
    if (L < 2 || L > 63) return 0;
    int lo = 0, hi = RC_MAX_LDS_BYTES / 8;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rc_encode_lds(mid, rc_split_segcap(mid)) <= RC_MAX_LDS_BYTES && rc_decode_lds(mid, L, rc_split_segcap(mid)) <= RC_MAX_LDS_BYTES) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

extern "C" size_t pccx_range_split_workspace_bytes(int B, int nsym, int seg_sym)
{
    if (B <= 0 || nsym < 0 || seg_sym < 1) return 0;
    const size_t P = (size_t)pccx_split_segments(nsym, seg_sym);
    const size_t enc = (size_t)B * P * 4 + (size_t)B * P * (size_t)rc_split_segcap(seg_sym), dec = (size_t)B * (P + 1) * 4;
    return ((enc > dec ? enc : dec) + 15) & ~(size_t)15;
}

extern "C" int pccx_split_stream_check_host(const uint8_t *bytes, int64_t nbytes, int nsym, int seg_sym, int segcap)
{
    if (nsym < 0 || seg_sym < 1 || segcap < 0 || (!bytes && nbytes > 0)) return PCCX_SPLIT_BAD_FIELDS;   // no file agrees with such a call
    return pccx_split_stream_check(bytes, nbytes, nsym, seg_sym, segcap, nullptr);
}

__global__ __launch_bounds__(64) void range_encode_split_kernel(const int32_t *__restrict__ cdf_int, const float *__restrict__ latent_q,
                                                                int nsym, int seg_sym, int P, int Lp, int sym_offset,
                                                                uint8_t *__restrict__ rows, int segcap, int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
    const int p = blockIdx.x, b = blockIdx.y;
    const int first = p * seg_sym;                                     // < nsym: p < P
    const int n = nsym - first < seg_sym ? nsym - first : seg_sym;     // ragged last segment
    const size_t row = (size_t)b * P + p;
    rc_encode_wave(rc_smem, cdf_int + ((size_t)b * nsym + first) * Lp, latent_q + (size_t)b * nsym + first, n, Lp, sym_offset,
                   rows + row * segcap, segcap, counts + row);
}

// One cloud per blockIdx.x, gridDim.y workgroups share its segments.  Every workgroup scans the cloud's P counts (256 partial sums of
// P/256 consecutive counts each), the first writes the header, and wave w of workgroup y copies segments y*4 + w, + 4*gridDim.y, ...
// 64 consecutive bytes per store instruction.  Nothing is written at or after `cap`.  A count that overflowed its scratch row (a
// table with zero-width symbols, outside the coder's contract) is copied as far as it was written and marks the cloud negative.
#define RC_PACK_THREADS 256
__global__ __launch_bounds__(RC_PACK_THREADS) void range_split_pack_kernel(const uint8_t *__restrict__ rows, const int32_t *__restrict__ counts,
                                                                          int nsym, int seg_sym, int P, int segcap,
                                                                          uint8_t *__restrict__ out, int cap, int32_t *__restrict__ nbytes)
{
    __shared__ int s_off[PCCX_SPLIT_MAX_SEGMENTS + 1];                 // segment offsets in the file
    __shared__ long long s_part[RC_PACK_THREADS];
    __shared__ int s_bad;
    const int b = blockIdx.x, t = threadIdx.x;
    const int32_t *cnt = counts + (size_t)b * P;
    uint8_t *o = out + (size_t)b * cap;
    const int per = (P + RC_PACK_THREADS - 1) / RC_PACK_THREADS;
    const int p0 = t * per < P ? t * per : P, p1 = p0 + per < P ? p0 + per : P;
    if (t == 0) s_bad = 0;
    __syncthreads();
    long long sum = 0;
    int bad = 0;
    for (int p = p0; p < p1; ++p) {
        const int c = cnt[p];
        bad |= c < 0;
        sum += c < 0 ? -(long long)c : c;
    }
    s_part[t] = sum;
    if (bad) s_bad = 1;
    __syncthreads();
    const long long header = PCCX_SPLIT_HEADER_BYTES + 2ll * P;
    long long off = header;
    for (int i = 0; i < t; ++i) off += s_part[i];
    for (int p = p0; p < p1; ++p) {
        s_off[p] = (int)(off < cap ? off : cap);                       // clamped: what lies at or after cap is not written
        const int c = cnt[p];
        off += c < 0 ? -(long long)c : c;
    }
    if (t == RC_PACK_THREADS - 1) {
        // the last thread's running sum is the file length (p1 = P for it, or its range is empty and every range before it ends at P)
        s_off[P] = (int)(off < cap ? off : cap);
        if (blockIdx.y == 0) nbytes[b] = (off <= cap && !s_bad && off <= 0x7FFFFFFFll) ? (int)off : -(int)(off < 0x7FFFFFFFll ? off : 0x7FFFFFFFll);
    }
    __syncthreads();
    if (blockIdx.y == 0) {
        for (int i = t; i < header && i < cap; i += RC_PACK_THREADS) {
            unsigned v;
            if (i < 4) v = i == 0 ? 'P' : i == 1 ? 'X' : i == 2 ? 'S' : '1';
            else if (i < 8) v = ((unsigned)nsym >> (8 * (i - 4))) & 0xFFu;
            else if (i < 10) v = ((unsigned)seg_sym >> (8 * (i - 8))) & 0xFFu;
            else if (i < 12) v = 0u;
            else {
                const int c = cnt[(i - 12) >> 1];
                const unsigned len = (unsigned)(c < 0 ? (-(long long)c > 0xFFFF ? 0xFFFF : -c) : c);
                v = (len >> (8 * (i & 1))) & 0xFFu;
            }
            o[i] = (uint8_t)v;
        }
    }
    const int wave = t >> 6, lane = t & 63;
    for (int p = blockIdx.y * (RC_PACK_THREADS / 64) + wave; p < P; p += gridDim.y * (RC_PACK_THREADS / 64)) {
        const int c = cnt[p];
        int len = c < 0 ? segcap : c;                                  // an overflowed row holds segcap bytes
        len = len > segcap ? segcap : len;
        const int at = s_off[p];
        if (len > cap - at) len = cap - at;                            // at <= cap
        const uint8_t *src = rows + ((size_t)b * P + p) * segcap;
        for (int i = lane; i < len; i += 64) o[at + i] = src[i];
    }
}

__global__ __launch_bounds__(64) void range_split_check_kernel(const uint8_t *__restrict__ in, int stride, const int32_t *__restrict__ nbytes,
                                                               int B, int nsym, int seg_sym, int P, int segcap,
                                                               int32_t *__restrict__ status, int32_t *__restrict__ offsets)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    // a count beyond the row is cut to the row before anything is read: such a file then fails its own length sum (status 3)
    const int nb = rc_row_bytes(nbytes[b], stride);
    status[b] = pccx_split_stream_check(in + (size_t)b * stride, nb, nsym, seg_sym, segcap, offsets + (size_t)b * (P + 1));
}

// The segment a wave of the per-segment decoders (grid (waves, B)) takes: which one of cloud blockIdx.y (p), its symbol count (n: the
// last segment may be ragged) and its first table / output row.  Two cases:
//   LIST = false (whole batch) : wave blockIdx.x takes segment blockIdx.x, rows in place at b * nsym + p * seg_sym;
//   LIST = true (region decode): wave j takes segment seg_idx[j], cut into [0, P), of ONE cloud (B = 1), rows compact at j * seg_sym.
// Either way only that segment's bytes are read, so no byte of an unlisted segment is touched.  LIST is a template argument and
// seg_idx the kernels' last argument, so that the whole-batch kernels keep their instructions and the place of their decode loop: a
// run-time test of seg_idx in front of it cost the indexed decoder 5 us of 280 (128 segments of 1024 symbols).
struct RcSegment {
    int p, n, first;                                                   // first = p * seg_sym, the segment's first symbol of its cloud
};
template <bool LIST>
__device__ __forceinline__ RcSegment rc_segment(const int32_t *__restrict__ seg_idx, int nsym, int seg_sym, int P)
{
    RcSegment s;
    s.p = blockIdx.x;
    if (LIST) {
        const int p = (int)rc_uni((unsigned)seg_idx[blockIdx.x]);
        s.p = p < 0 ? 0 : (p > P - 1 ? P - 1 : p);
    }
    s.first = s.p * seg_sym;                                           // < nsym: p < P
    s.n = nsym - s.first < seg_sym ? nsym - s.first : seg_sym;
    return s;
}
// its rows of an array of `width` words per symbol (the tables: L + 1, the output: 1), formed where they are addressed
template <bool LIST, class T>
__device__ __forceinline__ T *rc_segment_rows(T *base, const RcSegment &s, int nsym, int seg_sym, int width)
{
    const int j = blockIdx.x, b = blockIdx.y;
    return LIST ? base + (size_t)j * seg_sym * width : base + ((size_t)b * nsym + s.first) * width;
}

template <bool LIST>
__global__ __launch_bounds__(64) void range_decode_split_kernel(const int32_t *__restrict__ cdf_int, const uint8_t *__restrict__ in, int stride,
                                                                const int32_t *__restrict__ offsets, int nsym, int seg_sym, int P, int Lp,
                                                                int sym_offset, int segcap, float *__restrict__ latent_q,
                                                                const int32_t *__restrict__ seg_idx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
    const int b = blockIdx.y;
    const RcSegment s = rc_segment<LIST>(seg_idx, nsym, seg_sym, P);
    const int32_t *off = offsets + (size_t)b * (P + 1) + s.p;
    // the check kernel's offsets: 0 <= off[0] <= off[1] <= min(nbytes, stride), lengths <= segcap on status 0 and 0 otherwise; the
    // clamps restate that here, where the addresses are formed
    int at = (int)rc_uni((unsigned)off[0]), end = (int)rc_uni((unsigned)off[1]);
    at = at < 0 ? 0 : (at > stride ? stride : at);
    end = end < at ? at : (end > stride ? stride : end);
    const int nb = end - at > segcap ? segcap : end - at;
    rc_decode_wave(rc_smem, rc_segment_rows<LIST>(cdf_int, s, nsym, seg_sym, Lp), in + (size_t)b * stride + at, segcap, nb, s.n, Lp, sym_offset,
                   rc_segment_rows<LIST>(latent_q, s, nsym, seg_sym, 1));
}

// Both split decoders: the check kernel (status per cloud, offsets in workspace), then one wave per segment; seg_idx null: whole batch.
static int rc_decode_split_launch(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, int B, int nsym, int seg_sym,
                                  int L, const int32_t *seg_idx, int n_waves, float *latent_q, int32_t *status, void *workspace,
                                  hipStream_t stream)
{
    const int P = (int)pccx_split_segments(nsym, seg_sym), segcap = rc_split_segcap(seg_sym);
    int32_t *offsets = (int32_t *)workspace;
    hipLaunchKernelGGL(range_split_check_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, in, stride, nbytes, B, nsym, seg_sym, P, segcap,
                       status, offsets);
    PCCX_CHECK_LAUNCH();
    if (n_waves > 0) {
        const auto kernel = seg_idx ? range_decode_split_kernel<true> : range_decode_split_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(n_waves, B), dim3(64),
                           rc_decode_lds(seg_sym, L, segcap), stream, cdf_int, in, stride, offsets, nsym, seg_sym, P, L + 1, L / 2, segcap,
                           latent_q, seg_idx);
        PCCX_CHECK_LAUNCH();
    }
    return PCCX_OK;
}

static int rc_split_check_args(const char *who, int B, int nsym, int seg_sym, int L)
{
    PCCX_CHECK_ARG(B >= 0 && B <= 65535 && nsym >= 0 && seg_sym >= 1, "%s: bad shape (B=%d, nsym=%d, seg_sym=%d)", who, B, nsym, seg_sym);
    PCCX_CHECK_ARG(L >= 2 && L <= 63, "%s: L=%d; the wave kernels take 2 <= L <= 63", who, L);
    PCCX_CHECK_ARG(seg_sym <= pccx_range_split_max_seg_sym(L),
                   "%s: seg_sym=%d does not fit the %d bytes of LDS a segment is staged in; the largest seg_sym at L=%d is %d", who, seg_sym,
                   RC_MAX_LDS_BYTES, L, pccx_range_split_max_seg_sym(L));
    PCCX_CHECK_ARG(pccx_split_segments(nsym, seg_sym) <= PCCX_SPLIT_MAX_SEGMENTS, "%s: %lld segments; at most %d (nsym=%d, seg_sym=%d)", who,
                   (long long)pccx_split_segments(nsym, seg_sym), PCCX_SPLIT_MAX_SEGMENTS, nsym, seg_sym);
    return PCCX_OK;
}

extern "C" int pccx_range_encode_split(const int32_t *cdf_int, const float *latent_q, int B, int nsym, int seg_sym, int L, uint8_t *out,
                                       int cap, int32_t *nbytes, void *workspace, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    const int rc = rc_split_check_args("pccx_range_encode_split", B, nsym, seg_sym, L);
    if (rc != PCCX_OK) return rc;
    const int P = (int)pccx_split_segments(nsym, seg_sym), segcap = rc_split_segcap(seg_sym);
    PCCX_CHECK_ARG(out && nbytes && (nsym == 0 || (cdf_int && latent_q && workspace)), "pccx_range_encode_split: null pointer");
    PCCX_CHECK_ARG(cap >= 8, "pccx_range_encode_split: bad shape (cap=%d)", cap);
    int32_t *counts = (int32_t *)workspace;
    uint8_t *rows = (uint8_t *)workspace + (size_t)B * P * 4;
    if (P > 0) {
        hipLaunchKernelGGL(range_encode_split_kernel, dim3(P, B), dim3(64), rc_encode_lds(seg_sym, segcap), (hipStream_t)stream, cdf_int,
                           latent_q, nsym, seg_sym, P, L + 1, L / 2, rows, segcap, counts);
        PCCX_CHECK_LAUNCH();
    }
    const int slices = P > 4 * 64 ? 64 : (P + 3) / 4 > 0 ? (P + 3) / 4 : 1;
    hipLaunchKernelGGL(range_split_pack_kernel, dim3(B, slices), dim3(RC_PACK_THREADS), 0, (hipStream_t)stream, rows, counts, nsym, seg_sym, P,
                       segcap, out, cap, nbytes);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

extern "C" int pccx_range_decode_split(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, int B, int nsym,
                                       int seg_sym, int L, float *latent_q, int32_t *status, void *workspace, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    const int rc = rc_split_check_args("pccx_range_decode_split", B, nsym, seg_sym, L);
    if (rc != PCCX_OK) return rc;
    PCCX_CHECK_ARG(in && nbytes && status && workspace && (nsym == 0 || (cdf_int && latent_q)), "pccx_range_decode_split: null pointer");
    PCCX_CHECK_ARG(stride >= 1, "pccx_range_decode_split: bad shape (stride=%d)", stride);
    return rc_decode_split_launch(cdf_int, in, stride, nbytes, B, nsym, seg_sym, L, nullptr, (int)pccx_split_segments(nsym, seg_sym), latent_q,
                                  status, workspace, (hipStream_t)stream);
}

extern "C" int pccx_range_decode_split_list(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, int nsym,
                                            int seg_sym, int L, const int32_t *seg_idx, int n_list, float *latent_q, int32_t *status,
                                            void *workspace, void *stream)
{
    const int rc = rc_split_check_args("pccx_range_decode_split_list", 1, nsym, seg_sym, L);
    if (rc != PCCX_OK) return rc;
    const int P = (int)pccx_split_segments(nsym, seg_sym);
    PCCX_CHECK_ARG(n_list >= 0 && n_list <= P, "pccx_range_decode_split_list: %d segments listed of %d", n_list, P);
    PCCX_CHECK_ARG(in && nbytes && status && workspace && (n_list == 0 || (cdf_int && latent_q && seg_idx)),
                   "pccx_range_decode_split_list: null pointer");
    PCCX_CHECK_ARG(stride >= 1, "pccx_range_decode_split_list: bad shape (stride=%d)", stride);
    return rc_decode_split_launch(cdf_int, in, stride, nbytes, 1, nsym, seg_sym, L, seg_idx, n_list, latent_q, status, workspace,
                                  (hipStream_t)stream);
}

// ---- entry-point index: any number of waves enter the ONE stream of a cloud side by side -------------------------------------
// Format and check: entry_index.h.  The stream is pccx_range_encode's, byte for byte; the sidecar holds the coder's state at every
// seg_sym boundary.  Encode = the sequential encoder (wave or one lane, as pccx_range_coder_form says) that also stores the entries;
// build = the sequential decoder doing the same on an existing stream; decode = one check kernel per call (status per cloud + 4 words
// per segment in workspace), then every segment by rc_decode_wave<INIT> from its entry, staging only the bytes between its position
// and the next one's plus the 32-bit window: at most rc_index_stage bytes (maxspan + 32 bits starting inside a byte).
static int rc_index_maxspan(int seg_sym) { return 8 * rc_split_segcap(seg_sym); }        // bits a segment may shift in
static int rc_index_stage(int seg_sym) { return rc_split_segcap(seg_sym) + 8; }

extern "C" size_t pccx_range_index_bytes(int nsym, int seg_sym)
{
    if (nsym < 0 || seg_sym < 1) return 0;
    return (size_t)pccx_index_bytes(nsym, seg_sym);
}

extern "C" size_t pccx_range_index_workspace_bytes(int B, int nsym, int seg_sym)
{
    if (B <= 0 || nsym < 0 || seg_sym < 1) return 0;
    return (((size_t)B * (size_t)pccx_index_segments(nsym, seg_sym) * PCCX_INDEX_SEG_WORDS * 4) + 15) & ~(size_t)15;
}

extern "C" int pccx_entry_index_check_host(const uint8_t *index, int64_t idx_bytes, int64_t stream_bytes, int nsym, int seg_sym)
{
    if (nsym < 0 || seg_sym < 1 || seg_sym > (1 << 24) || idx_bytes < 0 || stream_bytes < 0 || stream_bytes > 0x7FFFFFFFll || (!index && idx_bytes > 0))
        return PCCX_INDEX_BAD_FIELDS;                                   // no file agrees with such a call
    return pccx_entry_index_check(index, idx_bytes, stream_bytes, nsym, seg_sym, rc_index_maxspan(seg_sym), nullptr);
}

__global__ __launch_bounds__(64) void range_encode_indexed_wave_kernel(const int32_t *__restrict__ cdf_int, const float *__restrict__ latent_q,
                                                                       int nsym, int Lp, int sym_offset, uint8_t *__restrict__ out, int cap,
                                                                       int32_t *__restrict__ nbytes, int seg_sym, uint8_t *__restrict__ index,
                                                                       int idx_stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
    const int b = blockIdx.x;
    uint32_t *side = (uint32_t *)(index + (size_t)b * idx_stride);
    if (threadIdx.x == 0) rc_index_header(side, nsym, seg_sym);
    rc_encode_wave<true>(rc_smem, cdf_int + (size_t)b * nsym * Lp, latent_q + (size_t)b * nsym, nsym, Lp, sym_offset, out + (size_t)b * cap,
                         cap, nbytes + b, side + PCCX_INDEX_HEADER_BYTES / 4, seg_sym);
}

__global__ __launch_bounds__(64) void range_index_build_wave_kernel(const int32_t *__restrict__ cdf_int, const uint8_t *__restrict__ in,
                                                                    int stride, const int32_t *__restrict__ nbytes, int nsym, int Lp,
                                                                    int sym_offset, float *__restrict__ latent_q, int seg_sym,
                                                                    uint8_t *__restrict__ index, int idx_stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
    const int b = blockIdx.x;
    const int nb = rc_row_bytes(nbytes[b], stride);
    uint32_t *side = (uint32_t *)(index + (size_t)b * idx_stride);
    if (threadIdx.x == 0) rc_index_header(side, nsym, seg_sym);
    rc_decode_wave<false, true>(rc_smem, cdf_int + (size_t)b * nsym * Lp, in + (size_t)b * stride, stride, nb, nsym, Lp, sym_offset,
                                latent_q ? latent_q + (size_t)b * nsym : nullptr, 0u, 0xFFFFFFFFu, 0, false,
                                side + PCCX_INDEX_HEADER_BYTES / 4, seg_sym);
}

__global__ __launch_bounds__(64) void range_index_check_kernel(const uint8_t *__restrict__ index, int idx_stride, const int32_t *__restrict__ idx_nbytes,
                                                               int stride, const int32_t *__restrict__ nbytes, int B, int nsym, int seg_sym,
                                                               int P, int maxspan, int32_t *__restrict__ status, uint32_t *__restrict__ seg)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    // counts beyond their rows are cut to the rows before anything is read
    const int nb = rc_row_bytes(nbytes[b], stride);
    const int ni = !idx_nbytes ? idx_stride : rc_row_bytes(idx_nbytes[b], idx_stride);
    status[b] = pccx_entry_index_check(index + (size_t)b * idx_stride, ni, nb, nsym, seg_sym, maxspan, seg + (size_t)b * P * PCCX_INDEX_SEG_WORDS);
}

// Segment p of one cloud from the check kernel's four words, decoded into q.  in / nbrow: the cloud's row and its byte count cut to
// the row.  The check gives pos <= end <= 8 * nbrow and end - pos <= maxspan + 32 (all 0 on a refused sidecar); the clamps restate
// that here, where the addresses are formed: the bytes read are in[at .. at + nb) with 0 <= at <= at + nb <= nbrow and nb <= stage.
__device__ __forceinline__ void rc_decode_entry(unsigned char *smem, const int32_t *__restrict__ c, const uint8_t *__restrict__ in, int nbrow,
                                                const uint32_t *__restrict__ seg, int stage, int n, int Lp, int sym_offset,
                                                float *__restrict__ q)
{
    const unsigned low = rc_uni(seg[0]), high = rc_uni(seg[1]), pf = rc_uni(seg[2]), end = rc_uni(seg[3]);
    const unsigned pos = pf & ~PCCX_INDEX_FLAG;
    int at = (int)(pos >> 3);                                          // < 2^28
    const unsigned endb = (end >> 3) + ((end & 7u) ? 1u : 0u);         // < 2^29 + 1
    int to = endb > (unsigned)nbrow ? nbrow : (int)endb;
    at = at > nbrow ? nbrow : at;
    to = to < at ? at : to;
    const int nb = to - at > stage ? stage : to - at;
    rc_decode_wave<true>(smem, c, in + at, stage, nb, n, Lp, sym_offset, q, low, high, (int)(pos & 7u), (pf & PCCX_INDEX_FLAG) != 0u);
}

template <bool LIST>
__global__ __launch_bounds__(64) void range_decode_indexed_kernel(const int32_t *__restrict__ cdf_int, const uint8_t *__restrict__ in, int stride,
                                                                  const int32_t *__restrict__ nbytes, const uint32_t *__restrict__ seg,
                                                                  int nsym, int seg_sym, int P, int Lp, int sym_offset, int stage,
                                                                  float *__restrict__ latent_q, const int32_t *__restrict__ seg_idx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
    const int b = blockIdx.y;
    const RcSegment s = rc_segment<LIST>(seg_idx, nsym, seg_sym, P);
    const int nbrow = rc_row_bytes((int)rc_uni((unsigned)nbytes[b]), stride);
    rc_decode_entry(rc_smem, rc_segment_rows<LIST>(cdf_int, s, nsym, seg_sym, Lp), in + (size_t)b * stride, nbrow,
                    seg + ((size_t)b * P + s.p) * PCCX_INDEX_SEG_WORDS, stage, s.n, Lp, sym_offset,
                    rc_segment_rows<LIST>(latent_q, s, nsym, seg_sym, 1));
}

// Both indexed decoders: the check kernel (status per cloud, four words per segment in workspace), then one wave per segment.
// idx_nbytes null: every sidecar is idx_stride bytes.  seg_idx null: the whole batch.
static int rc_decode_indexed_launch(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, const uint8_t *index,
                                    int idx_stride, const int32_t *idx_nbytes, int B, int nsym, int seg_sym, int L, const int32_t *seg_idx,
                                    int n_waves, float *latent_q, int32_t *status, void *workspace, hipStream_t stream)
{
    const int P = (int)pccx_index_segments(nsym, seg_sym), stage = rc_index_stage(seg_sym);
    uint32_t *seg = (uint32_t *)workspace;
    hipLaunchKernelGGL(range_index_check_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, index, idx_stride, idx_nbytes, stride, nbytes, B,
                       nsym, seg_sym, P, rc_index_maxspan(seg_sym), status, seg);
    PCCX_CHECK_LAUNCH();
    if (n_waves > 0) {
        const auto kernel = seg_idx ? range_decode_indexed_kernel<true> : range_decode_indexed_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(n_waves, B), dim3(64),
                           rc_decode_lds(seg_sym, L, stage), stream, cdf_int, in, stride, nbytes, seg, nsym, seg_sym, P, L + 1, L / 2, stage,
                           latent_q, seg_idx);
        PCCX_CHECK_LAUNCH();
    }
    return PCCX_OK;
}

// The shapes every indexed entry point takes: those of the split path, and a stream whose bit positions fit the 31 bits of an entry.
static int rc_index_check_args(const char *who, int B, int nsym, int seg_sym, int L, int64_t stream_bytes)
{
    const int rc = rc_split_check_args(who, B, nsym, seg_sym, L);
    if (rc != PCCX_OK) return rc;
    PCCX_CHECK_ARG(stream_bytes >= 1 && stream_bytes <= (1 << 27), "%s: a stream row of %lld bytes; 1 .. 2^27 (bit positions are 31 bits wide)", who,
                   (long long)stream_bytes);
    return PCCX_OK;
}

extern "C" int pccx_range_encode_indexed(const int32_t *cdf_int, const float *latent_q, int B, int nsym, int seg_sym, int L, uint8_t *out,
                                         int cap, int32_t *nbytes, uint8_t *index, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    const int rc = rc_index_check_args("pccx_range_encode_indexed", B, nsym, seg_sym, L, cap);
    if (rc != PCCX_OK) return rc;
    PCCX_CHECK_ARG(cdf_int && latent_q && out && nbytes && index, "pccx_range_encode_indexed: null pointer");
    PCCX_CHECK_ARG(cap >= 8 && ((uintptr_t)index & 3) == 0, "pccx_range_encode_indexed: bad shape (cap=%d) or an index that is not 4-byte aligned", cap);
    const int idx_stride = (int)pccx_index_bytes(nsym, seg_sym);
    if (pccx_range_coder_form(0, nsym, L, cap) == 0) {
        hipLaunchKernelGGL(range_encode_indexed_wave_kernel, dim3(B), dim3(64), rc_encode_lds(nsym, cap), (hipStream_t)stream, cdf_int, latent_q,
                           nsym, L + 1, L / 2, out, cap, nbytes, seg_sym, index, idx_stride);
        PCCX_CHECK_LAUNCH();
        return PCCX_OK;
    }
    hipLaunchKernelGGL(range_encode_indexed_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cdf_int, latent_q, B, nsym, L + 1,
                       L / 2, out, cap, nbytes, seg_sym, index, idx_stride);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

extern "C" int pccx_range_index_build(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, int B, int nsym,
                                      int seg_sym, int L, uint8_t *index, float *latent_q, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    const int rc = rc_index_check_args("pccx_range_index_build", B, nsym, seg_sym, L, stride);
    if (rc != PCCX_OK) return rc;
    PCCX_CHECK_ARG(cdf_int && in && nbytes && index, "pccx_range_index_build: null pointer");
    PCCX_CHECK_ARG(((uintptr_t)index & 3) == 0, "pccx_range_index_build: an index that is not 4-byte aligned");
    const int idx_stride = (int)pccx_index_bytes(nsym, seg_sym);
    if (pccx_range_coder_form(1, nsym, L, stride) == 0) {
        hipLaunchKernelGGL(range_index_build_wave_kernel, dim3(B), dim3(64), rc_decode_lds(nsym, L, stride), (hipStream_t)stream, cdf_int, in,
                           stride, nbytes, nsym, L + 1, L / 2, latent_q, seg_sym, index, idx_stride);
        PCCX_CHECK_LAUNCH();
        return PCCX_OK;
    }
    hipLaunchKernelGGL(range_index_build_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cdf_int, in, stride, nbytes, B, nsym,
                       L + 1, L / 2, latent_q, seg_sym, index, idx_stride);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}

extern "C" int pccx_range_decode_indexed(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, const uint8_t *index,
                                         int idx_stride, const int32_t *idx_nbytes, int B, int nsym, int seg_sym, int L, float *latent_q,
                                         int32_t *status, void *workspace, void *stream)
{
    if (B == 0) return PCCX_OK;   // empty batch: nothing to do, pointers may be null
    const int rc = rc_index_check_args("pccx_range_decode_indexed", B, nsym, seg_sym, L, stride);
    if (rc != PCCX_OK) return rc;
    PCCX_CHECK_ARG(in && nbytes && index && status && workspace && (nsym == 0 || (cdf_int && latent_q)), "pccx_range_decode_indexed: null pointer");
    PCCX_CHECK_ARG(idx_stride >= 0, "pccx_range_decode_indexed: bad shape (idx_stride=%d)", idx_stride);
    return rc_decode_indexed_launch(cdf_int, in, stride, nbytes, index, idx_stride, idx_nbytes, B, nsym, seg_sym, L, nullptr,
                                    (int)pccx_index_segments(nsym, seg_sym), latent_q, status, workspace, (hipStream_t)stream);
}

extern "C" int pccx_range_decode_indexed_list(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes,
                                              const uint8_t *index, int idx_bytes, int nsym, int seg_sym, int L, const int32_t *seg_idx,
                                              int n_list, float *latent_q, int32_t *status, void *workspace, void *stream)
{
    const int rc = rc_index_check_args("pccx_range_decode_indexed_list", 1, nsym, seg_sym, L, stride);
    if (rc != PCCX_OK) return rc;
    const int P = (int)pccx_index_segments(nsym, seg_sym);
    PCCX_CHECK_ARG(n_list >= 0 && n_list <= P, "pccx_range_decode_indexed_list: %d segments listed of %d", n_list, P);
    PCCX_CHECK_ARG(in && nbytes && index && status && workspace && (n_list == 0 || (cdf_int && latent_q && seg_idx)),
                   "pccx_range_decode_indexed_list: null pointer");
    PCCX_CHECK_ARG(idx_bytes >= 0, "pccx_range_decode_indexed_list: bad shape (idx_bytes=%d)", idx_bytes);
    return rc_decode_indexed_launch(cdf_int, in, stride, nbytes, index, idx_bytes, nullptr, 1, nsym, seg_sym, L, seg_idx, n_list, latent_q,
                                    status, workspace, (hipStream_t)stream);
}

// torchac's float -> 16-bit CDF conversion (torchac 0.9.3 _convert_to_int_and_normalize, needs_normalization=True; the
// same formula as prob_forward_kernel's epilogue): cdf_int[l] = (round(cdf[l] * (2^16 - (Lp - 1))) + l) mod 2^16.
__global__ void cdf_float_to_int_kernel(const float *__restrict__ cdf, int64_t n, int Lp, int32_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int l = (int)(i % Lp);
    out[i] = ((int)rintf(__fmul_rn(cdf[i], (float)(65536 - (Lp - 1)))) + l) & 0xFFFF;
}

extern "C" int pccx_cdf_float_to_int(const float *cdf, int64_t nrows, int Lp, int32_t *cdf_int, void *stream)
{
    if (nrows == 0) return PCCX_OK;
    PCCX_CHECK_ARG(cdf && cdf_int, "pccx_cdf_float_to_int: null pointer");
    PCCX_CHECK_ARG(nrows > 0 && Lp >= 2 && Lp <= 65536, "pccx_cdf_float_to_int: bad shape");
    const int64_t n = nrows * Lp;
    hipLaunchKernelGGL(cdf_float_to_int_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cdf, n, Lp, cdf_int);
    PCCX_CHECK_LAUNCH();
    return PCCX_OK;
}
