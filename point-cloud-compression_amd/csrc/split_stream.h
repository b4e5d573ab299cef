// split_stream.h -- the header rules of a split range-coded latent stream (.p.bin in split form), stated once for the host
// (pccx_split_stream_check_host, the CLIs) and the device (the check kernel in front of the split decoder).  Plain C++ with no
// dependency, so that it also compiles alone with a host compiler.
//
//   magic "PXS1" | nsym u32 | seg_sym u16 | reserved u16 = 0 | len[P] u16, P = ceil(nsym / seg_sym) | the P segment streams
//
// (all little-endian).  This function is all that stands between a foreign file and the decoder's addresses:
//   * it reads byte i only after i + 1 <= nbytes has been established (the 12 fixed bytes after nbytes >= 12, the directory after
//     12 + 2P <= nbytes), whatever the bytes say;
//   * every offset it yields is min(running sum, nbytes), so 0 <= off[p] <= off[p+1] <= nbytes for all p, and on any status but 0
//     all P + 1 offsets are 0: every segment is then empty and the decoder forms no address from the file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCCX_SPLIT_HD __host__ __device__
#else
#define PCCX_SPLIT_HD
#endif

#define PCCX_SPLIT_HEADER_BYTES 12
#define PCCX_SPLIT_MAX_SEGMENTS 8192

enum {
    PCCX_SPLIT_OK = 0,
    PCCX_SPLIT_BAD_MAGIC = 1,      // shorter than its header, or the magic is wrong
    PCCX_SPLIT_BAD_FIELDS = 2,     // nsym / seg_sym / reserved disagree with the call
    PCCX_SPLIT_BAD_LENGTHS = 3     // a length above segcap, or header + sum of the lengths != nbytes
};

// Segments of a stream of nsym >= 0 symbols cut every seg_sym >= 1.
PCCX_SPLIT_HD static inline int64_t pccx_split_segments(int64_t nsym, int64_t seg_sym) { return (nsym + seg_sym - 1) / seg_sym; }

// Status of the nbytes bytes at `bytes` as the split stream of (nsym, seg_sym) whose segments take at most segcap bytes each.
// offsets: null, or P + 1 entries that receive where each segment starts and the last one ends (see above).  The caller's nsym,
// seg_sym and segcap are trusted (nsym >= 0, seg_sym >= 1, segcap >= 0; the entry points check them); the bytes are not.
PCCX_SPLIT_HD static inline int pccx_split_stream_check(const uint8_t *bytes, int64_t nbytes, int64_t nsym, int64_t seg_sym,
                                                        int64_t segcap, int32_t *offsets)
{
    const int64_t P = pccx_split_segments(nsym, seg_sym);
    const int64_t header = PCCX_SPLIT_HEADER_BYTES + 2 * P;
    int status = PCCX_SPLIT_OK;
    if (nbytes < PCCX_SPLIT_HEADER_BYTES || bytes[0] != 'P' || bytes[1] != 'X' || bytes[2] != 'S' || bytes[3] != '1')
        status = PCCX_SPLIT_BAD_MAGIC;
    else {
        const int64_t f_nsym = (int64_t)bytes[4] | (int64_t)bytes[5] << 8 | (int64_t)bytes[6] << 16 | (int64_t)bytes[7] << 24;
        const int64_t f_seg = (int64_t)bytes[8] | (int64_t)bytes[9] << 8;
        const int64_t f_res = (int64_t)bytes[10] | (int64_t)bytes[11] << 8;
        if (f_nsym != nsym || f_seg != seg_sym || f_res != 0)
            status = PCCX_SPLIT_BAD_FIELDS;
        else if (header > nbytes)
            status = PCCX_SPLIT_BAD_MAGIC;                              // shorter than its own directory
        else {
            int64_t off = header;                                       // header <= nbytes: the directory bytes below exist
            for (int64_t p = 0; p < P; ++p) {
                const int64_t len = (int64_t)bytes[PCCX_SPLIT_HEADER_BYTES + 2 * p] | (int64_t)bytes[PCCX_SPLIT_HEADER_BYTES + 2 * p + 1] << 8;
                if (len > segcap) status = PCCX_SPLIT_BAD_LENGTHS;
                if (offsets) offsets[p] = (int32_t)(off < nbytes ? off : nbytes);
                off += len;                                             // at most 12 + 2P + 65535 P: no overflow in 64 bits
            }
            if (offsets) offsets[P] = (int32_t)(off < nbytes ? off : nbytes);
            if (off != nbytes) status = PCCX_SPLIT_BAD_LENGTHS;
        }
    }
    if (status != PCCX_SPLIT_OK && offsets)
        for (int64_t p = 0; p <= P; ++p) offsets[p] = 0;
    return status;
}
