// entry_index.h -- the entry-point index of a single range-coded latent stream (<name>.p.idx beside the reference's .p.bin), stated
// once for the host (pccx_entry_index_check_host, the CLIs) and the device (the check kernel in front of the indexed decoder).  Plain
// C++ with no dependency, so that it also compiles alone with a host compiler.
//
//   magic "PXI1" | nsym u32 | seg_sym u32 | P u32 | P entries {low u32, high u32, pos u32},  P = ceil(nsym / seg_sym)
//
// (all little-endian).  Entry p is the decoder's state when it reaches symbol p*seg_sym: its interval, and in pos bits 0..30 the
// number of stream bits it has shifted in beyond its first 32, bit 31 set when an underflow run is pending there.  The decoder's
// `value` is not stored: it is the 32 stream bits from bit `pos` on, bit 31 inverted when the flag is set (rangecoder.hip,
// "bulk renormalisation").  Entry 0 is always {0, 0xFFFFFFFF, 0}.
//
// pccx_entry_index_check is all that stands between a foreign sidecar and the decoder's addresses:
//   * it reads byte i of the sidecar only after i + 1 <= idx_bytes has been established (the 16 fixed bytes after idx_bytes >= 16,
//     the entries after idx_bytes == 16 + 12 P), whatever the bytes say, and never reads the stream;
//   * what it yields per segment is {low, high, pos | flag, end} with pos <= end <= 8 * stream_bytes and end - pos <= maxspan + 32:
//     the decoder stages the bytes that hold stream bits [pos, end) and nothing else.  On any status but 0 every segment is
//     {0, 0xFFFFFFFF, 0, 0}: empty, so that the decoder forms no address from the stream.
// A sidecar that passes may still be wrong (it then decodes wrong symbols); it cannot move an address out of the staged bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCCX_INDEX_HD __host__ __device__
#else
#define PCCX_INDEX_HD
#endif

#define PCCX_INDEX_HEADER_BYTES 16
#define PCCX_INDEX_ENTRY_BYTES 12
#define PCCX_INDEX_SEG_WORDS 4         // what the check yields per segment: low, high, pos | flag, end
#define PCCX_INDEX_FLAG 0x80000000u

enum {
    PCCX_INDEX_OK = 0,
    PCCX_INDEX_BAD_MAGIC = 1,      // shorter than its header, the magic is wrong, or the length is not 16 + 12 P
    PCCX_INDEX_BAD_FIELDS = 2,     // nsym / seg_sym / P disagree with the call
    PCCX_INDEX_BAD_ORDER = 3,      // a position below the one before it
    PCCX_INDEX_BAD_POSITION = 4,   // a position beyond the stream's 8 * nbytes bits
    PCCX_INDEX_BAD_SPAN = 5,       // consecutive positions further apart than the bits a segment may take
    PCCX_INDEX_BAD_STATE = 6       // an interval the coder cannot be in after renormalisation, or entry 0 is not the initial state
};

PCCX_INDEX_HD static inline int64_t pccx_index_segments(int64_t nsym, int64_t seg_sym) { return (nsym + seg_sym - 1) / seg_sym; }
PCCX_INDEX_HD static inline int64_t pccx_index_bytes(int64_t nsym, int64_t seg_sym)
{
    return PCCX_INDEX_HEADER_BYTES + PCCX_INDEX_ENTRY_BYTES * pccx_index_segments(nsym, seg_sym);
}
PCCX_INDEX_HD static inline uint32_t pccx_index_u32(const uint8_t *p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
// The coder's interval after renormalisation: the top bits differ and no underflow step is left to take.
PCCX_INDEX_HD static inline int pccx_index_state_ok(uint32_t low, uint32_t high)
{
    return low < 0x80000000u && high >= 0x80000000u && !(low >= 0x40000000u && high < 0xC0000000u);
}

// Status of the idx_bytes bytes at `idx` as the index of (nsym, seg_sym) over a stream of stream_bytes bytes whose segments shift in
// at most maxspan bits each.  seg: null, or 4 words per segment (see above).  The caller's nsym >= 0, seg_sym >= 1,
// 0 <= stream_bytes < 2^31 and 0 <= maxspan < 2^31 - 32 are trusted (the entry points check them); the bytes are not.
PCCX_INDEX_HD static inline int pccx_entry_index_check(const uint8_t *idx, int64_t idx_bytes, int64_t stream_bytes, int64_t nsym,
                                                       int64_t seg_sym, int64_t maxspan, uint32_t *seg)
{
    const int64_t P = pccx_index_segments(nsym, seg_sym);
    const int64_t bits = 8 * stream_bytes;
    int status = PCCX_INDEX_OK;
    if (idx_bytes < PCCX_INDEX_HEADER_BYTES || idx[0] != 'P' || idx[1] != 'X' || idx[2] != 'I' || idx[3] != '1')
        status = PCCX_INDEX_BAD_MAGIC;
    else if ((int64_t)pccx_index_u32(idx + 4) != nsym || (int64_t)pccx_index_u32(idx + 8) != seg_sym || (int64_t)pccx_index_u32(idx + 12) != P)
        status = PCCX_INDEX_BAD_FIELDS;
    else if (idx_bytes != PCCX_INDEX_HEADER_BYTES + PCCX_INDEX_ENTRY_BYTES * P)
        status = PCCX_INDEX_BAD_MAGIC;                                  // truncated (or extended): not the P entries it announces
    else {
        int64_t prev = 0;                                               // all P entries exist: idx_bytes == 16 + 12 P
        for (int64_t p = 0; p < P; ++p) {
            const uint8_t *e = idx + PCCX_INDEX_HEADER_BYTES + PCCX_INDEX_ENTRY_BYTES * p;
            const uint32_t low = pccx_index_u32(e), high = pccx_index_u32(e + 4), pf = pccx_index_u32(e + 8);
            const int64_t pos = (int64_t)(pf & ~PCCX_INDEX_FLAG);
            int bad = PCCX_INDEX_OK;
            if (pos < prev) bad = PCCX_INDEX_BAD_ORDER;
            else if (pos > bits) bad = PCCX_INDEX_BAD_POSITION;
            else if (pos - prev > maxspan) bad = PCCX_INDEX_BAD_SPAN;
            else if (!pccx_index_state_ok(low, high) || (p == 0 && (low != 0u || high != 0xFFFFFFFFu || pf != 0u))) bad = PCCX_INDEX_BAD_STATE;
            if (status == PCCX_INDEX_OK) status = bad;
            if (seg) {
                seg[4 * p] = low, seg[4 * p + 1] = high, seg[4 * p + 2] = pf;
                if (p > 0) seg[4 * p - 1] = (uint32_t)(pos + 32 < bits ? pos + 32 : bits);     // the window after the last symbol
            }
            prev = pos;
        }
        if (seg && P > 0) seg[4 * P - 1] = (uint32_t)(prev + maxspan + 32 < bits ? prev + maxspan + 32 : bits);
    }
    if (status != PCCX_INDEX_OK && seg)
        for (int64_t p = 0; p < P; ++p) seg[4 * p] = 0u, seg[4 * p + 1] = 0xFFFFFFFFu, seg[4 * p + 2] = 0u, seg[4 * p + 3] = 0u;
    return status;
}
