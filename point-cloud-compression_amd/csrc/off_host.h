// off_host.h -- one OFF triangle mesh (the format of ModelNet40's CAD models), parsed from a byte buffer: its header into a plain
// struct, its body into float32 vertices and int32 faces.  Plain C++17 with no dependency (no HIP, nothing else of the project), as
// ply_host.h is: a host compiler builds it alone (tests/test_off_host_cpu.py does, under the address and undefined-behaviour sanitizers).
//
// Grammar (pccx/meshes.py read_off accepts and refuses the same files): '#' starts a comment, lines without a token are skipped, \r\n
// line ends are accepted.  The first token is OFF; the three counts nv nf ne stand behind it on the same line -- glued to it (OFF490 518
// 0, as many ModelNet40 files have it) or not -- or on the next line that has a token.  Then nv lines of three numbers (the token rule
// of ply_token_to_double: to double, then rounded to float32) and nf lines "3 a b c"; what follows the three indices (colours) is
// ignored.  Refused, each with a status and a message: see OffStatus.  A polygon is refused, not cut to its first three corners.
// Every index into the buffer is checked against its length: the bytes come from files of any origin.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <charconv>

enum OffStatus {
    OFF_OK = 0,
    OFF_NOT_OFF = 1,           // the first token does not begin with OFF
    OFF_TRUNCATED = 2,         // the buffer ends before the counts, or holds fewer lines than nv + nf
    OFF_BAD_NV = 3,            // nv outside 3 .. 2^31 - 1
    OFF_BAD_NF = 4,            // nf outside 1 .. 2^22
    OFF_NOT_TRIANGLE = 5,      // a face line that does not begin with 3
    OFF_BAD_INDEX = 6,         // a face index that is no number or lies outside 0 .. nv - 1, or fewer than three of them
    OFF_BAD_COORD = 7,         // a vertex line that does not hold three finite numbers
    OFF_MALFORMED = 8,         // a count line that does not hold three counts
    OFF_IO = 9,                // the file cannot be opened or read (set by hostio.hip)
    OFF_ARG = 10               // a staging range that does not hold the file (set by hostio.hip)
};

#define OFF_MAX_VERTICES 2147483647ll
#define OFF_MAX_FACES 4194304ll

struct OffHeader {
    int64_t nv, nf, ne;
    int64_t body_offset;       // first byte behind the line of the counts
};

namespace off_detail {

struct Tok {
    const uint8_t *p;
    size_t n;
};

// what str.split() splits on, for text decoded from ASCII
static inline bool space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f); }

// the first `cap` tokens of buf[a, b); returns how many there are (counting those beyond cap)
static inline size_t split(const uint8_t *buf, size_t a, size_t b, Tok *tok, size_t cap)
{
    size_t n = 0;
    while (a < b) {
        while (a < b && space(buf[a])) ++a;
        if (a >= b) break;
        size_t s = a;
        while (a < b && !space(buf[a])) ++a;
        if (n < cap) tok[n] = Tok{buf + s, a - s};
        ++n;
    }
    return n;
}

// a decimal count: optional '+', digits; -1 = not a count, -2 = above 2^31 - 1
static inline int64_t count(const Tok &t)
{
    size_t i = t.n && t.p[0] == '+' ? 1 : 0;
    if (i >= t.n) return -1;
    int64_t v = 0;
    bool over = false;
    for (; i < t.n; ++i) {
        if (t.p[i] < '0' || t.p[i] > '9') return -1;
        if (!over) v = v * 10 + (t.p[i] - '0');
        if (v > OFF_MAX_VERTICES) over = true;
    }
    return over ? -2 : v;
}

static inline int fail(int status, char *msg, size_t cap, const char *text)
{
    if (msg && cap) snprintf(msg, cap, "%s", text);
    return status;
}

// Lines of buf[pos, len): the next one that holds a token outside its comment -> [a, b) without the comment.  prefix: the buffer is the
// head of a longer file, so a last line without its '\n' is not a line yet.
struct Lines {
    const uint8_t *buf;
    size_t len, pos;
    bool prefix;
    bool next(size_t &a, size_t &b)
    {
        while (pos < len) {
            const void *nl = memchr(buf + pos, '\n', len - pos);
            if (!nl && prefix) return false;
            a = pos;
            b = nl ? (size_t)((const uint8_t *)nl - buf) : len;
            pos = nl ? b + 1 : len;
            const void *hash = memchr(buf + a, '#', b - a);
            if (hash) b = (size_t)((const uint8_t *)hash - buf);
            size_t i = a;
            while (i < b && space(buf[i])) ++i;
            if (i < b) return true;
        }
        return false;
    }
};

}  // namespace off_detail

// The header of the OFF file whose first `len` bytes are buf.  file_size: the file's length in bytes for the check that nv + nf lines
// can fit it, or -1 for no such check.  On any status but OFF_OK, *h is cleared and msg (msg_cap bytes, may be null) names the cause.
// With len < file_size the buffer is taken as a prefix of the file: only lines that end in it are parsed, and OFF_TRUNCATED means
// "hand me more of the file".
static inline int off_parse_header(const uint8_t *buf, size_t len, int64_t file_size, OffHeader *h, char *msg, size_t msg_cap)
{
    using namespace off_detail;
    memset(h, 0, sizeof(*h));
    if (msg && msg_cap) msg[0] = 0;
    if (!buf) len = 0;
    Lines ln{buf, len, 0, file_size > (int64_t)len};
    size_t a, b;
    Tok tok[5];
    if (!ln.next(a, b)) return fail(OFF_TRUNCATED, msg, msg_cap, "truncated: the file ends before its OFF line");
    size_t nt = split(buf, a, b, tok, 5);
    if (tok[0].n < 3 || memcmp(tok[0].p, "OFF", 3) != 0) return fail(OFF_NOT_OFF, msg, msg_cap, "not an OFF file");
    Tok cnt[3];
    size_t nc = 0;
    if (tok[0].n > 3) cnt[nc++] = Tok{tok[0].p + 3, tok[0].n - 3};               // OFF490 518 0
    for (size_t i = 1; i < nt; ++i) {
        if (nc >= 3 || i >= 5) return fail(OFF_MALFORMED, msg, msg_cap, "the OFF line holds more than three counts");
        cnt[nc++] = tok[i];
    }
    if (nc == 0) {
        if (!ln.next(a, b)) return fail(OFF_TRUNCATED, msg, msg_cap, "truncated: the file ends before its three counts");
        nt = split(buf, a, b, tok, 4);
        if (nt != 3) return fail(OFF_MALFORMED, msg, msg_cap, "the line of the counts does not hold three counts (nv nf ne)");
        for (nc = 0; nc < 3; ++nc) cnt[nc] = tok[nc];
    }
    if (nc != 3) return fail(OFF_MALFORMED, msg, msg_cap, "the OFF line does not hold three counts (nv nf ne)");
    const int64_t nv = count(cnt[0]), nf = count(cnt[1]), ne = count(cnt[2]);
    if (nv == -1 || nf == -1 || ne == -1) return fail(OFF_MALFORMED, msg, msg_cap, "a count (nv nf ne) is no number");
    if (nv < 3) return fail(OFF_BAD_NV, msg, msg_cap, "vertex count nv must be 3 .. 2147483647");
    if (nf < 1 || nf > OFF_MAX_FACES) return fail(OFF_BAD_NF, msg, msg_cap, "face count nf must be 1 .. 4194304");
    if (file_size >= 0) {
        // a vertex line takes six bytes at least ("0 0 0\n"), a face line eight ("3 0 0 0\n"), the last one may go without its '\n'
        const int64_t need = nv * 6 + nf * 8 - 1;                                // < 2^31 * 6 + 2^22 * 8: no overflow
        if ((int64_t)ln.pos > file_size || need > file_size - (int64_t)ln.pos)
            return fail(OFF_TRUNCATED, msg, msg_cap, "truncated: the file is too short for its counts");
    }
    h->nv = nv, h->nf = nf, h->ne = ne < 0 ? OFF_MAX_VERTICES : ne, h->body_offset = (int64_t)ln.pos;
    return OFF_OK;
}

// One token -> double: ply_host.h's ply_token_to_double, restated here because this header stands alone.  Decimal or exponent form, an
// optional sign, the whole token consumed, no locale; inf and nan parse too and are refused by the caller as non-finite.
static inline bool off_token_to_double(const uint8_t *p, size_t n, double *out)
{
    const char *s = (const char *)p, *e = s + n;
    if (s < e && *s == '+') {
        ++s;
        if (s < e && (*s == '+' || *s == '-')) return false;
    }
    if (s >= e) return false;
    for (const char *c = s; c < e; ++c)
        if (*c == '(') return false;
    const auto r = std::from_chars(s, e, *out, std::chars_format::general);
    if (r.ptr != e) return false;
    if (r.ec == std::errc::result_out_of_range) {      // strtod's answer: +-inf above the range, +-0 below it
        const bool neg = *s == '-';
        const char *c = s + (neg ? 1 : 0);
        int64_t lead = 0;                              // position of the first non-zero digit: > 0 in front of the point, <= 0 behind it
        bool point = false, found = false;
        for (; c < e && *c != 'e' && *c != 'E'; ++c) {
            if (*c == '.') point = true;
            else if (!found && *c != '0') found = true, lead += point ? 0 : 1;
            else if (found && !point) ++lead;
            else if (!found && point) --lead;
        }
        int64_t ex = 0;
        if (c < e) {
            ++c;
            const bool eneg = c < e && *c == '-';
            if (c < e && (*c == '-' || *c == '+')) ++c;
            for (; c < e && ex < 1000000000; ++c) ex = ex * 10 + (*c - '0');
            if (eneg) ex = -ex;
        }
        const double big = __builtin_huge_val();
        *out = lead + ex <= 0 ? (neg ? -0.0 : 0.0) : (neg ? -big : big);
        return true;
    }
    return r.ec == std::errc();
}

// The body text[0, len) of a mesh with header h (its bytes from h.body_offset on) -> verts (nv, 3) float32, faces (nf, 3) int32.  On
// any status but OFF_OK the two arrays hold nothing a caller may use.
static inline int off_parse_body(const uint8_t *text, size_t len, const OffHeader &h, float *verts, int32_t *faces, char *msg, size_t msg_cap)
{
    using namespace off_detail;
    if (msg && msg_cap) msg[0] = 0;
    if (!text) len = 0;
    Lines ln{text, len, 0, false};
    size_t a, b;
    Tok tok[4];
    for (int64_t i = 0; i < h.nv; ++i) {
        if (!ln.next(a, b)) return fail(OFF_TRUNCATED, msg, msg_cap, "truncated: fewer vertex lines than nv");
        if (split(text, a, b, tok, 4) != 3) return fail(OFF_BAD_COORD, msg, msg_cap, "a vertex line does not hold three numbers");
        for (int c = 0; c < 3; ++c) {
            double v;
            if (!off_token_to_double(tok[c].p, tok[c].n, &v)) return fail(OFF_BAD_COORD, msg, msg_cap, "a vertex line holds a token that is no number");
            const float f = (float)v;
            if (!isfinite(f)) return fail(OFF_BAD_COORD, msg, msg_cap, "a vertex coordinate is not finite as float32");
            verts[3 * i + c] = f;
        }
    }
    for (int64_t i = 0; i < h.nf; ++i) {
        if (!ln.next(a, b)) return fail(OFF_TRUNCATED, msg, msg_cap, "truncated: fewer face lines than nf");
        const size_t nt = split(text, a, b, tok, 4);
        const int64_t corners = count(tok[0]);
        if (corners == -1) return fail(OFF_BAD_INDEX, msg, msg_cap, "a face line does not begin with a count");
        if (corners != 3) return fail(OFF_NOT_TRIANGLE, msg, msg_cap, "a face is not a triangle (polygons are not triangulated)");
        if (nt < 4) return fail(OFF_BAD_INDEX, msg, msg_cap, "a face line holds fewer than three indices");
        for (int c = 0; c < 3; ++c) {
            const int64_t v = count(tok[1 + c]);
            if (v < 0 || v >= h.nv) return fail(OFF_BAD_INDEX, msg, msg_cap, "a face index is no number or lies outside 0 .. nv - 1");
            faces[3 * i + c] = (int32_t)v;
        }
    }
    return OFF_OK;
}
