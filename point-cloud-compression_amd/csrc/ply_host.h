// ply_host.h -- the header of one PLY file, parsed from a byte buffer into a plain struct, and the text-to-float rule of its ASCII
// form.  Plain C++17 with no dependency (no HIP, nothing else of the project), as split_stream.h and entry_index.h are: a host compiler
// builds it alone (tests/test_ply_host_cpu.py does, under the address and undefined-behaviour sanitizers).
//
// It accepts what pccx/plyio.py read_point_cloud accepts -- the sixteen type names of _TYPES, x y z or X Y Z (the lower-case name wins
// per coordinate), any other scalar vertex properties in any position, comment / obj_info / unknown and blank lines, \r\n line ends,
// further elements BEHIND the vertex element -- and refuses, naming the cause, what that reader refuses or silently misreads: see
// PlyStatus.  Every index into the buffer is checked against its length: the bytes come from files of any origin.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <charconv>
#include <vector>

enum PlyStatus {
    PLY_OK = 0,
    PLY_NOT_PLY = 1,           // the first line is not "ply"
    PLY_TRUNCATED = 2,         // the buffer ends before end_header
    PLY_BAD_FORMAT = 3,        // no format line, or not ascii / binary_little_endian / binary_big_endian
    PLY_BAD_TYPE = 4,          // a vertex property of a type outside plyio._TYPES
    PLY_LIST = 5,              // a list property on the vertex element
    PLY_MISSING_COORD = 6,     // no x / X, y / Y or z / Z
    PLY_NO_VERTEX = 7,         // no vertex element
    PLY_ELEMENT_ORDER = 8,     // an element in front of vertex (its bytes would be read as vertices), or vertex declared twice
    PLY_BAD_COUNT = 9,         // n_vertex below 1 or above 2^31 - 1
    PLY_STRIDE = 10,           // a record of more than PLY_MAX_STRIDE bytes
    PLY_SIZE = 11,             // n_vertex records do not fit the file
    PLY_MALFORMED = 12,        // a header line that lacks a token, or a property name declared twice in a binary file
    PLY_IO = 13,               // the file cannot be opened or read (set by hostio.hip)
    PLY_ROWS = 14,             // an ASCII file with fewer than n_vertex complete rows, or a token that is no number
    PLY_ARG = 15               // a staging range that does not hold the file (set by hostio.hip)
};

enum { PLY_ASCII = 0, PLY_LE = 1, PLY_BE = 2 };
// type codes, in the order of their sizes' table below: int8 uint8 int16 uint16 int32 uint32 float32 float64
enum { PLY_I1 = 0, PLY_U1, PLY_I2, PLY_U2, PLY_I4, PLY_U4, PLY_F4, PLY_F8, PLY_NTYPES };
#define PLY_MAX_STRIDE 4096
#define PLY_MAX_VERTICES 2147483647ll

static inline int ply_type_size(int code)
{
    static const int size[PLY_NTYPES] = {1, 1, 2, 2, 4, 4, 4, 8};
    return code >= 0 && code < PLY_NTYPES ? size[code] : 0;
}

struct PlyHeader {
    int format;                // PLY_ASCII / PLY_LE / PLY_BE
    int n_props;               // scalar properties of the vertex element (the tokens of one ASCII row)
    int64_t n_vertex;
    int64_t stride;            // bytes of one binary record
    int64_t data_offset;       // first byte behind the end_header line
    int off[3], type[3];       // byte offset inside a record and type code of x, y, z
    int col[3];                // their property indices (the columns of an ASCII row)
};

namespace ply_detail {

struct Tok {
    const uint8_t *p;
    size_t n;
    bool is(const char *s) const { return strlen(s) == n && memcmp(p, s, n) == 0; }
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

static inline int type_code(const Tok &t)
{
    static const struct { const char *name; int code; } names[16] = {
        {"char", PLY_I1}, {"int8", PLY_I1}, {"uchar", PLY_U1}, {"uint8", PLY_U1}, {"short", PLY_I2}, {"int16", PLY_I2},
        {"ushort", PLY_U2}, {"uint16", PLY_U2}, {"int", PLY_I4}, {"int32", PLY_I4}, {"uint", PLY_U4}, {"uint32", PLY_U4},
        {"float", PLY_F4}, {"float32", PLY_F4}, {"double", PLY_F8}, {"float64", PLY_F8}};
    for (const auto &e : names)
        if (t.is(e.name)) return e.code;
    return -1;
}

// a decimal count: optional '+', digits; -1 = not a count, -2 = above PLY_MAX_VERTICES (a negative count reads as "not a count")
static inline int64_t count(const Tok &t)
{
    size_t i = t.n && t.p[0] == '+' ? 1 : 0;
    if (i >= t.n) return -1;
    int64_t v = 0;
    bool over = false;
    for (; i < t.n; ++i) {
        if (t.p[i] < '0' || t.p[i] > '9') return -1;
        if (!over) v = v * 10 + (t.p[i] - '0');
        if (v > PLY_MAX_VERTICES) over = true;
    }
    return over ? -2 : v;
}

static inline int fail(int status, char *msg, size_t cap, const char *text)
{
    if (msg && cap) snprintf(msg, cap, "%s", text);
    return status;
}

}  // namespace ply_detail

// The header of the PLY file whose first `len` bytes are buf.  file_size: the file's length in bytes for the check that the vertex
// block fits it, or -1 for no such check.  On any status but PLY_OK, *h is cleared and msg (msg_cap bytes, may be null) names the cause.
// With len < file_size the buffer is taken as a prefix of the file: only lines that end in it are parsed, and PLY_TRUNCATED means
// "hand me more of the file".
static inline int ply_parse_header(const uint8_t *buf, size_t len, int64_t file_size, PlyHeader *h, char *msg, size_t msg_cap)
{
    using namespace ply_detail;
    memset(h, 0, sizeof(*h));
    if (msg && msg_cap) msg[0] = 0;
    if (!buf) len = 0;
    size_t pos = 0;
    // one line = up to and including the next '\n', or the rest of the FILE: where the buffer is a prefix of a longer file, a last line
    // without its '\n' may be cut anywhere, inside a type name for instance, and is not a line yet
    const bool prefix = file_size > (int64_t)len;
    auto next_line = [&](size_t &a, size_t &b) {
        if (pos >= len) return false;
        const void *nl = memchr(buf + pos, '\n', len - pos);
        if (!nl && prefix) return false;
        a = pos;
        b = nl ? (size_t)((const uint8_t *)nl - buf) + 1 : len;
        pos = b;
        return true;
    };
    size_t a, b;
    Tok tok[4];
    // (a first line that does not end inside 64 bytes is not "ply", however much of the file follows)
    if (!next_line(a, b)) return prefix && len < 64 ? fail(PLY_TRUNCATED, msg, msg_cap, "truncated header") : fail(PLY_NOT_PLY, msg, msg_cap, "not a PLY file");
    if (split(buf, a, b, tok, 4) != 1 || !tok[0].is("ply")) return fail(PLY_NOT_PLY, msg, msg_cap, "not a PLY file");
    int format = -1, n_props = 0;
    bool have_format = false, in_vertex = false, seen_vertex = false, seen_other = false, ended = false;
    int64_t n_vertex = 0, stride = 0;
    struct Prop { Tok name; int type; int64_t off; };
    std::vector<Prop> props;
    while (next_line(a, b)) {
        const size_t nt = split(buf, a, b, tok, 4);
        if (nt == 0) continue;
        if (tok[0].is("format")) {
            if (nt < 2) return fail(PLY_MALFORMED, msg, msg_cap, "format line without a format");
            have_format = true;
            format = tok[1].is("ascii") ? PLY_ASCII : tok[1].is("binary_little_endian") ? PLY_LE : tok[1].is("binary_big_endian") ? PLY_BE : -1;
        } else if (tok[0].is("element")) {
            if (nt < 2) return fail(PLY_MALFORMED, msg, msg_cap, "element line without a name");
            in_vertex = tok[1].is("vertex");
            if (in_vertex) {
                if (seen_vertex) return fail(PLY_ELEMENT_ORDER, msg, msg_cap, "vertex element declared twice");
                if (seen_other) return fail(PLY_ELEMENT_ORDER, msg, msg_cap, "an element is declared in front of vertex: its data would be read as vertices");
                if (nt < 3) return fail(PLY_MALFORMED, msg, msg_cap, "element vertex without a count");
                seen_vertex = true;
                n_vertex = count(tok[2]);
                if (n_vertex < 1) return fail(PLY_BAD_COUNT, msg, msg_cap, "vertex count must be 1 .. 2147483647");
            } else {
                seen_other = true;
            }
        } else if (tok[0].is("property") && in_vertex) {
            if (nt < 2) return fail(PLY_MALFORMED, msg, msg_cap, "property line without a type");
            if (tok[1].is("list")) return fail(PLY_LIST, msg, msg_cap, "list property on vertex element unsupported");
            const int t = type_code(tok[1]);
            if (t < 0) return fail(PLY_BAD_TYPE, msg, msg_cap, "unknown property type on the vertex element");
            if (nt < 3) return fail(PLY_MALFORMED, msg, msg_cap, "property line without a name");
            props.push_back(Prop{tok[2], t, stride});
            stride += ply_type_size(t);
            ++n_props;
            if (stride > PLY_MAX_STRIDE) return fail(PLY_STRIDE, msg, msg_cap, "vertex record longer than 4096 bytes");
        } else if (tok[0].is("end_header")) {
            ended = true;
            break;
        }
    }
    if (!ended) return fail(PLY_TRUNCATED, msg, msg_cap, "truncated header");
    if (!have_format) return fail(PLY_BAD_FORMAT, msg, msg_cap, "no format line");
    if (format < 0) return fail(PLY_BAD_FORMAT, msg, msg_cap, "unsupported PLY format");
    if (!seen_vertex) return fail(PLY_NO_VERTEX, msg, msg_cap, "no vertex element");
    // a name declared twice has no meaning as a field of a binary record (read_point_cloud's structured dtype refuses it); in an ASCII
    // file that reader takes the first column of the name, as the search below does.  Checked on a sorted copy: there may be thousands.
    if (format != PLY_ASCII) {
        std::vector<Tok> names;
        names.reserve(props.size());
        for (const Prop &p : props) names.push_back(p.name);
        auto less = [](const Tok &x, const Tok &y) {
            const int c = memcmp(x.p, y.p, std::min(x.n, y.n));
            return c < 0 || (c == 0 && x.n < y.n);
        };
        std::sort(names.begin(), names.end(), less);
        for (size_t i = 1; i < names.size(); ++i)
            if (!less(names[i - 1], names[i])) return fail(PLY_MALFORMED, msg, msg_cap, "a vertex property name is declared twice");
    }
    const char *lower[3] = {"x", "y", "z"}, *upper[3] = {"X", "Y", "Z"};
    for (int c = 0; c < 3; ++c) {
        int at = -1;
        for (size_t i = 0; i < props.size() && at < 0; ++i)
            if (props[i].name.is(lower[c])) at = (int)i;
        for (size_t i = 0; i < props.size() && at < 0; ++i)
            if (props[i].name.is(upper[c])) at = (int)i;
        if (at < 0) return fail(PLY_MISSING_COORD, msg, msg_cap, "the vertex element has no x, y and z (or X, Y and Z)");
        h->col[c] = at, h->off[c] = (int)props[at].off, h->type[c] = props[at].type;
    }
    h->format = format, h->n_props = n_props, h->n_vertex = n_vertex, h->stride = stride, h->data_offset = (int64_t)pos;
    if (file_size >= 0) {
        // binary: n records; ASCII: every token takes a byte and a separator, the last one may go without
        const int64_t need = format == PLY_ASCII ? n_vertex * (2 * (int64_t)n_props) - 1 : n_vertex * stride;   // < 2^31 * 8192: no overflow
        if ((int64_t)pos > file_size || need > file_size - (int64_t)pos) {
            memset(h, 0, sizeof(*h));
            return fail(PLY_SIZE, msg, msg_cap, "the file is too short for its vertex count");
        }
    }
    return PLY_OK;
}

// One token of an ASCII row -> double, as np.loadtxt's float converter reads it: decimal or exponent form, an optional sign, inf /
// infinity / nan in any letter case; the whole token must be consumed.  No locale takes part.  The caller rounds the double to float:
// two roundings, as loadtxt followed by astype(float32) makes -- one rounding from the text differs in the last bit on some inputs.
static inline bool ply_token_to_double(const uint8_t *p, size_t n, double *out)
{
    const char *s = (const char *)p, *e = s + n;
    if (s < e && *s == '+') {
        ++s;
        if (s < e && (*s == '+' || *s == '-')) return false;
    }
    if (s >= e) return false;
    for (const char *c = s; c < e; ++c)
        if (*c == '(') return false;                   // from_chars reads nan(payload); Python's float does not
    const auto r = std::from_chars(s, e, *out, std::chars_format::general);
    if (r.ptr != e) return false;
    if (r.ec == std::errc::result_out_of_range) {      // strtod's answer: +-inf above the range, +-0 below it
        // from_chars leaves *out alone here.  The sign of the decimal exponent of the leading non-zero digit tells which side it is.
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

// The first n_vertex complete rows of the ASCII vertex block text[0, len) -> out (n_vertex, 3) float32 x, y, z.  A row is a line
// with tokens ('#' starts a comment, as in np.loadtxt; blank lines are skipped) and holds exactly h.n_props numbers.
static inline int ply_parse_ascii_rows(const uint8_t *text, size_t len, const PlyHeader &h, float *out, char *msg, size_t msg_cap)
{
    using namespace ply_detail;
    std::vector<Tok> tok((size_t)h.n_props);
    size_t pos = 0;
    int64_t row = 0;
    while (row < h.n_vertex && pos < len) {
        const void *nl = memchr(text + pos, '\n', len - pos);
        size_t a = pos, b = nl ? (size_t)((const uint8_t *)nl - text) : len;
        pos = nl ? b + 1 : len;
        const void *hash = memchr(text + a, '#', b - a);
        if (hash) b = (size_t)((const uint8_t *)hash - text);
        const size_t nt = split(text, a, b, tok.data(), tok.size());
        if (nt == 0) continue;
        if (nt != (size_t)h.n_props) return fail(PLY_ROWS, msg, msg_cap, "an ASCII vertex row does not hold one number per property");
        for (int c = 0; c < 3; ++c) {
            double v;
            const Tok &t = tok[(size_t)h.col[c]];
            if (!ply_token_to_double(t.p, t.n, &v)) return fail(PLY_ROWS, msg, msg_cap, "an ASCII vertex row holds a token that is no number");
            out[3 * row + c] = (float)v;
        }
        ++row;
    }
    if (row < h.n_vertex) return fail(PLY_ROWS, msg, msg_cap, "fewer complete ASCII rows than the header's vertex count");
    return PLY_OK;
}
