// hostio.hip -- the three files of every cloud, written from / read into the packed stream buffer of one batch (pccx/codec.py
// packed_layout) by a small pool of host threads.  Pure host code (no HIP call): compress.py:139-152 writes <name>.p.bin, <name>.s.bin and
// <name>.c.bin INSIDE its timer and decompress.py:80-91,113 reads them back inside its own, one open/write/close per file from Python;
// for a batch of 1024 clouds that is 6144 small-file operations per step, 70 ms of interpreter time (gpurun_out/r3d/files.json) beside a
// 37 ms GPU step.  Here a batch's files are cut from the ONE host copy of the packed buffer (the bytes are never re-assembled per cloud)
// by threads that share an atomic cloud counter.  Formats are the reference's: .s.bin = the first s_nbytes[b] bytes
// of row b of s_bytes, .p.bin = the first p_nbytes[b] bytes of row b of p_bytes, .c.bin = 16 bytes [cx, cy, cz, longest] fp32.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "off_host.h"
#include "ply_host.h"

namespace {

// byte offsets of the five sections (codec.packed_layout): s_nbytes (B) i32 | p_nbytes (B) i32 | c (B,4) f32 | s_bytes (B,s_stride) |
// p_bytes (B,p_cap)
struct Layout {
    size_t sn, pn, c, sb, pb, end;
    Layout(int B, int s_stride, int p_cap)
    {
        sn = 0, pn = 4 * (size_t)B, c = 8 * (size_t)B, sb = c + 16 * (size_t)B;
        pb = sb + (size_t)B * s_stride, end = pb + (size_t)B * p_cap;
    }
};

// A pool that lives as long as the process (allocated once, never destroyed: its threads sleep on the condition variable at exit).
// run(n, threads, fn): fn(i) for every i < n, on `threads` threads counting the caller; returns when all are done.
class Pool {
public:
    static Pool &get()
    {
        static Pool *p = new Pool();
        return *p;
    }
    void run(int n, int threads, const std::function<void(int)> &fn)
    {
        if (threads > n) threads = n;
        if (threads <= 1) {
            for (int i = 0; i < n; ++i) fn(i);
            return;
        }
        std::unique_lock<std::mutex> call(call_mu_);          // one batch at a time
        grow(threads - 1);
        {
            std::lock_guard<std::mutex> g(mu_);
            fn_ = &fn, n_ = n, next_.store(0), want_ = threads - 1, running_ = 0, ++epoch_;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [&] { return want_ == 0 && running_ == 0; });
        fn_ = nullptr;
    }

private:
    void work()
    {
        for (int i; (i = next_.fetch_add(1)) < n_;) (*fn_)(i);
    }
    void grow(int workers)
    {
        while ((int)th_.size() < workers) {
            th_.emplace_back([this] {
                uint64_t seen = 0;
                for (;;) {
                    {
                        std::unique_lock<std::mutex> g(mu_);
                        cv_.wait(g, [&] { return epoch_ != seen && want_ > 0; });
                        seen = epoch_, --want_, ++running_;
                    }
                    work();
                    {
                        std::lock_guard<std::mutex> g(mu_);
                        --running_;
                    }
                    done_.notify_all();
                }
            });
            th_.back().detach();
        }
    }
    std::mutex call_mu_, mu_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> th_;
    const std::function<void(int)> *fn_ = nullptr;
    std::atomic<int> next_{0};
    int n_ = 0, want_ = 0, running_ = 0;
    uint64_t epoch_ = 0;
};

int default_threads()
{
    unsigned hw = std::thread::hardware_concurrency();
    return hw == 0 ? 4 : (hw > 8 ? 8 : (int)hw);
}

// head (may be empty) and then buf into one file
bool write_all(const char *path, const void *buf, size_t len, std::string &err, const void *head = nullptr, size_t head_len = 0)
{
    // an existing file first: O_CREAT makes the kernel take the DIRECTORY's lock exclusively for the lookup, which serialises the
    // threads of a batch that rewrites one directory (the steady state of a codec loop)
    int fd = open(path, O_WRONLY | O_TRUNC | O_CLOEXEC);
    if (fd < 0 && errno == ENOENT) fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) {
        err = std::string("open ") + path + ": " + strerror(errno);
        return false;
    }
    for (int part = 0; part < 2; ++part) {
        const char *p = (const char *)(part ? buf : head);
        size_t left = part ? len : head_len;
        while (left > 0) {
            ssize_t w = write(fd, p, left);
            if (w < 0) {
                if (errno == EINTR) continue;
                err = std::string("write ") + path + ": " + strerror(errno);
                close(fd);
                return false;
            }
            p += w, left -= (size_t)w;
        }
    }
    if (close(fd) != 0) {
        err = std::string("close ") + path + ": " + strerror(errno);
        return false;
    }
    return true;
}

// the whole file into buf (at most cap bytes): its length, or -1 (error / larger than cap)
long read_all(const char *path, void *buf, size_t cap, std::string &err)
{
    int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) {
        err = std::string("open ") + path + ": " + strerror(errno);
        return -1;
    }
    size_t got = 0;
    char *p = (char *)buf;
    char extra;
    for (;;) {
        ssize_t r = got < cap ? read(fd, p + got, cap - got) : read(fd, &extra, 1);
        if (r < 0) {
            if (errno == EINTR) continue;
            err = std::string("read ") + path + ": " + strerror(errno);
            close(fd);
            return -1;
        }
        if (r == 0) break;
        if (got >= cap) {
            err = std::string(path) + ": longer than the " + std::to_string(cap) + " bytes the stream buffer holds per cloud";
            close(fd);
            return -1;
        }
        got += (size_t)r;
    }
    close(fd);
    return (long)got;
}

struct Names {
    const char *dir, *names;
    const int64_t *off;
    std::string path(int b, const char *ext) const
    {
        std::string s(dir);
        if (!s.empty() && s.back() != '/') s.push_back('/');
        s += names + off[b];
        s += ext;
        return s;
    }
};

int check_common(const void *packed, int B, int s_stride, int p_cap, const char *dir, const char *names, const int64_t *off, const char *who)
{
    PCCX_CHECK_ARG(packed && dir && names && off, "%s: null pointer", who);
    PCCX_CHECK_ARG(B >= 0 && s_stride >= 0 && p_cap >= 0, "%s: negative size", who);
    return PCCX_OK;
}

}  // namespace

extern "C" int pccx_write_streams_host(const void *packed_host, int B, int s_stride, int p_cap, const char *dir, const char *names,
                                       const int64_t *name_off, int threads)
{
    int rc = check_common(packed_host, B, s_stride, p_cap, dir, names, name_off, "pccx_write_streams_host");
    if (rc != PCCX_OK) return rc;
    const Layout L(B, s_stride, p_cap);
    const uint8_t *base = (const uint8_t *)packed_host;
    const int32_t *sn = (const int32_t *)(base + L.sn), *pn = (const int32_t *)(base + L.pn);
    for (int b = 0; b < B; ++b)      // a negative count is the coder's "output buffer too small" (rangecoder.hip): nothing is written
        PCCX_CHECK_ARG(sn[b] >= 0 && sn[b] <= s_stride && pn[b] >= 0 && pn[b] <= p_cap,
                       "pccx_write_streams_host: cloud %d has byte counts %d / %d outside its rows of %d / %d bytes (a negative count "
                       "means the coder's output buffer was too small)", b, sn[b], pn[b], s_stride, p_cap);
    const Names nm{dir, names, name_off};
    std::mutex emu;
    std::string first;
    Pool::get().run(B, threads > 0 ? threads : default_threads(), [&](int b) {
        std::string err;
        // the reference's order (compress.py:139-152): .p.bin, .s.bin, .c.bin
        bool ok = write_all(nm.path(b, ".p.bin").c_str(), base + L.pb + (size_t)b * p_cap, (size_t)pn[b], err) &&
                  write_all(nm.path(b, ".s.bin").c_str(), base + L.sb + (size_t)b * s_stride, (size_t)sn[b], err) &&
                  write_all(nm.path(b, ".c.bin").c_str(), base + L.c + 16 * (size_t)b, 16, err);
        if (!ok) {
            std::lock_guard<std::mutex> g(emu);
            if (first.empty()) first = err;
        }
    });
    if (!first.empty()) {
        pccx_set_error("pccx_write_streams_host: %s", first.c_str());
        return PCCX_ERR_ARG;
    }
    return PCCX_OK;
}

extern "C" int pccx_read_streams_host(void *packed_host, int B, int s_stride, int p_cap, const char *dir, const char *names,
                                      const int64_t *name_off, int threads)
{
    int rc = check_common(packed_host, B, s_stride, p_cap, dir, names, name_off, "pccx_read_streams_host");
    if (rc != PCCX_OK) return rc;
    const Layout L(B, s_stride, p_cap);
    uint8_t *base = (uint8_t *)packed_host;
    int32_t *sn = (int32_t *)(base + L.sn), *pn = (int32_t *)(base + L.pn);
    const Names nm{dir, names, name_off};
    std::mutex emu;
    std::string first;
    Pool::get().run(B, threads > 0 ? threads : default_threads(), [&](int b) {
        std::string err;
        // the reference's order (decompress.py:80-91,113): .s.bin, .p.bin, .c.bin
        long s = read_all(nm.path(b, ".s.bin").c_str(), base + L.sb + (size_t)b * s_stride, (size_t)s_stride, err);
        long p = s < 0 ? -1 : read_all(nm.path(b, ".p.bin").c_str(), base + L.pb + (size_t)b * p_cap, (size_t)p_cap, err);
        long c = p < 0 ? -1 : read_all(nm.path(b, ".c.bin").c_str(), base + L.c + 16 * (size_t)b, 16, err);
        if (c >= 0 && c != 16) err = nm.path(b, ".c.bin") + ": " + std::to_string(c) + " bytes, expected the 16 of [cx, cy, cz, longest]", c = -1;
        if (c < 0) {
            sn[b] = pn[b] = 0;
            std::lock_guard<std::mutex> g(emu);
            if (first.empty()) first = err;
            return;
        }
        sn[b] = (int32_t)s, pn[b] = (int32_t)p;
        // rows are handed to the decoders whole: clear what the files did not fill
        memset(base + L.sb + (size_t)b * s_stride + s, 0, (size_t)s_stride - (size_t)s);
        memset(base + L.pb + (size_t)b * p_cap + p, 0, (size_t)p_cap - (size_t)p);
    });
    if (!first.empty()) {
        pccx_set_error("pccx_read_streams_host: %s", first.c_str());
        return PCCX_ERR_ARG;
    }
    return PCCX_OK;
}

extern "C" int pccx_stream_sizes_host(int B, const char *dir, const char *names, const int64_t *name_off, int64_t *s_sizes, int64_t *p_sizes,
                                      int threads)
{
    PCCX_CHECK_ARG(dir && names && name_off && s_sizes && p_sizes, "pccx_stream_sizes_host: null pointer");
    PCCX_CHECK_ARG(B >= 0, "pccx_stream_sizes_host: negative size");
    const Names nm{dir, names, name_off};
    Pool::get().run(B, threads > 0 ? threads : default_threads(), [&](int b) {
        struct stat st;
        s_sizes[b] = stat(nm.path(b, ".s.bin").c_str(), &st) == 0 ? (int64_t)st.st_size : -1;
        p_sizes[b] = stat(nm.path(b, ".p.bin").c_str(), &st) == 0 ? (int64_t)st.st_size : -1;
    });
    return PCCX_OK;
}

// The sidecars of the entry-point index (entry_index.h), one <name>.p.idx per cloud, beside the three files and by the same threads.
// They are rows of their own (B, idx_stride): the packed layout of the three streams does not change.
extern "C" int pccx_write_index_host(const void *index_host, int B, int idx_stride, const char *dir, const char *names, const int64_t *name_off,
                                     int threads)
{
    PCCX_CHECK_ARG(index_host && dir && names && name_off, "pccx_write_index_host: null pointer");
    PCCX_CHECK_ARG(B >= 0 && idx_stride >= 0, "pccx_write_index_host: negative size");
    const uint8_t *base = (const uint8_t *)index_host;
    const Names nm{dir, names, name_off};
    std::mutex emu;
    std::string first;
    Pool::get().run(B, threads > 0 ? threads : default_threads(), [&](int b) {
        std::string err;
        if (!write_all(nm.path(b, ".p.idx").c_str(), base + (size_t)b * idx_stride, (size_t)idx_stride, err)) {
            std::lock_guard<std::mutex> g(emu);
            if (first.empty()) first = err;
        }
    });
    if (!first.empty()) {
        pccx_set_error("pccx_write_index_host: %s", first.c_str());
        return PCCX_ERR_ARG;
    }
    return PCCX_OK;
}

extern "C" int pccx_read_index_host(void *index_host, int B, int idx_stride, int32_t *idx_nbytes, const char *dir, const char *names,
                                    const int64_t *name_off, int threads)
{
    PCCX_CHECK_ARG(index_host && idx_nbytes && dir && names && name_off, "pccx_read_index_host: null pointer");
    PCCX_CHECK_ARG(B >= 0 && idx_stride >= 0, "pccx_read_index_host: negative size");
    uint8_t *base = (uint8_t *)index_host;
    const Names nm{dir, names, name_off};
    std::mutex emu;
    std::string first;
    Pool::get().run(B, threads > 0 ? threads : default_threads(), [&](int b) {
        std::string err;
        const long n = read_all(nm.path(b, ".p.idx").c_str(), base + (size_t)b * idx_stride, (size_t)idx_stride, err);
        if (n < 0) {
            idx_nbytes[b] = 0;
            std::lock_guard<std::mutex> g(emu);
            if (first.empty()) first = err;
            return;
        }
        idx_nbytes[b] = (int32_t)n;
        memset(base + (size_t)b * idx_stride + n, 0, (size_t)idx_stride - (size_t)n);
    });
    if (!first.empty()) {
        pccx_set_error("pccx_read_index_host: %s", first.c_str());
        return PCCX_ERR_ARG;
    }
    return PCCX_OK;
}

// ---- PLY files on the same threads: scan the headers of a batch into a table, load every vertex block raw into
// one staging buffer (pccx_ply_unpack, csrc/plyio.hip, converts it on the GPU), write reconstructions.  A row of the table is
// PCCX_PLY_ROW int64: status, format, n_vertex, stride, data offset, file size, byte offset of x y z, type code of x y z, properties
// per record, property index of x y z (ply_host.h: PlyStatus, PlyHeader).  A file that fails keeps its status in the row and its cause
// in msgs (B, msg_stride) chars; the others are still done, so the caller can name every bad file at once.
namespace {

void ply_row_fail(int64_t *row, char *msg, int msg_stride, int status, const std::string &text)
{
    row[0] = status;
    if (msg && msg_stride > 0) snprintf(msg, (size_t)msg_stride, "%s", text.c_str());
}

void ply_row_set(int64_t *row, const PlyHeader &h, int64_t file_size)
{
    row[0] = PLY_OK, row[1] = h.format, row[2] = h.n_vertex, row[3] = h.stride, row[4] = h.data_offset, row[5] = file_size;
    for (int c = 0; c < 3; ++c) row[6 + c] = h.off[c], row[9 + c] = h.type[c], row[13 + c] = h.col[c];
    row[12] = h.n_props;
}

// exactly len bytes from offset at; false with err set on an error or a short file
bool pread_all(int fd, void *buf, size_t len, int64_t at, std::string &err)
{
    char *p = (char *)buf;
    while (len > 0) {
        ssize_t r = pread(fd, p, len, (off_t)at);
        if (r < 0) {
            if (errno == EINTR) continue;
            err = std::string("read: ") + strerror(errno);
            return false;
        }
        if (r == 0) {
            err = "the file ends inside its vertex block";
            return false;
        }
        p += r, len -= (size_t)r, at += r;
    }
    return true;
}

void ply_scan_one(const char *path, int64_t *row, char *msg, int msg_stride)
{
    for (int j = 0; j < PCCX_PLY_ROW; ++j) row[j] = 0;
    if (msg && msg_stride > 0) msg[0] = 0;
    int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return ply_row_fail(row, msg, msg_stride, PLY_IO, std::string("open: ") + strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
        close(fd);
        return ply_row_fail(row, msg, msg_stride, PLY_IO, "not a regular file");
    }
    const int64_t size = (int64_t)st.st_size;
    row[5] = size;
    std::vector<uint8_t> buf;
    PlyHeader h;
    char text[160];
    int status = PLY_TRUNCATED;
    // most headers fit the first 4 KiB; one that does not is read again, four times as far, up to 16 MiB
    for (int64_t want = 4096; status == PLY_TRUNCATED; want *= 4) {
        const size_t len = (size_t)(want < size ? want : size);
        buf.resize(len);
        std::string err;
        if (len && !pread_all(fd, buf.data(), len, 0, err)) {
            close(fd);
            return ply_row_fail(row, msg, msg_stride, PLY_IO, err);
        }
        status = ply_parse_header(buf.data(), len, size, &h, text, sizeof(text));
        if ((int64_t)len >= size || want >= (16ll << 20)) break;
    }
    close(fd);
    if (status != PLY_OK) return ply_row_fail(row, msg, msg_stride, status, text);
    ply_row_set(row, h, size);
}

void ply_load_one(const char *path, int64_t *row, uint8_t *staging, int64_t staging_bytes, int64_t dst, char *msg, int msg_stride)
{
    const int64_t format = row[1], n = row[2], stride = row[3], at = row[4], size = row[5];
    const bool ascii = format == PLY_ASCII;
    // the row is the caller's memory: nothing in it is trusted further than the scan's own limits
    if (n < 1 || n > PLY_MAX_VERTICES || stride < 1 || stride > PLY_MAX_STRIDE || at < 0 || size < at || (format != PLY_ASCII && format != PLY_LE && format != PLY_BE))
        return ply_row_fail(row, msg, msg_stride, PLY_ARG, "a table row that pccx_ply_scan_host did not fill");
    const int64_t need = n * (ascii ? 12 : stride);
    if (dst < 0 || dst % 16 != 0 || dst > staging_bytes || need > staging_bytes - dst)
        return ply_row_fail(row, msg, msg_stride, PLY_ARG, "the staging range of this file is not 16-byte aligned or does not hold its " + std::to_string(need) + " bytes");
    int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return ply_row_fail(row, msg, msg_stride, PLY_IO, std::string("open: ") + strerror(errno));
    std::string err;
    if (!ascii) {
        const bool ok = pread_all(fd, staging + dst, (size_t)need, at, err);
        close(fd);
        if (!ok) return ply_row_fail(row, msg, msg_stride, PLY_IO, err);
        return;
    }
    PlyHeader h;
    memset(&h, 0, sizeof(h));
    h.format = PLY_ASCII, h.n_vertex = n, h.n_props = (int)row[12];
    for (int c = 0; c < 3; ++c) h.col[c] = (int)row[13 + c];
    if (row[12] < 3 || row[12] > PLY_MAX_STRIDE || h.col[0] < 0 || h.col[1] < 0 || h.col[2] < 0 || h.col[0] >= h.n_props || h.col[1] >= h.n_props ||
        h.col[2] >= h.n_props) {
        close(fd);
        return ply_row_fail(row, msg, msg_stride, PLY_ARG, "a table row that pccx_ply_scan_host did not fill");
    }
    std::vector<uint8_t> text((size_t)(size - at));
    const bool ok = text.empty() || pread_all(fd, text.data(), text.size(), at, err);
    close(fd);
    if (!ok) return ply_row_fail(row, msg, msg_stride, PLY_IO, err);
    char why[160];
    const int status = ply_parse_ascii_rows(text.data(), text.size(), h, (float *)(staging + dst), why, sizeof(why));
    if (status != PLY_OK) return ply_row_fail(row, msg, msg_stride, status, why);
    // what the staging range now holds: float32 x y z records
    row[1] = PLY_LE, row[3] = 12;
    for (int c = 0; c < 3; ++c) row[6 + c] = 4 * c, row[9 + c] = PLY_F4;
}

}  // namespace

extern "C" int pccx_ply_scan_host(int B, const char *paths, const int64_t *path_off, int64_t *table, char *msgs, int msg_stride, int threads)
{
    PCCX_CHECK_ARG(B >= 0 && msg_stride >= 0, "pccx_ply_scan_host: negative size");
    if (B == 0) return PCCX_OK;
    PCCX_CHECK_ARG(paths && path_off && table && (msgs || msg_stride == 0), "pccx_ply_scan_host: null pointer");
    Pool::get().run(B, threads > 0 ? threads : default_threads(), [&](int b) {
        ply_scan_one(paths + path_off[b], table + (size_t)b * PCCX_PLY_ROW, msgs ? msgs + (size_t)b * msg_stride : nullptr, msg_stride);
    });
    return PCCX_OK;
}

extern "C" int pccx_ply_load_host(int B, const char *paths, const int64_t *path_off, int64_t *table, void *staging_host, int64_t staging_bytes,
                                  const int64_t *dst_off, char *msgs, int msg_stride, int threads)
{
    PCCX_CHECK_ARG(B >= 0 && msg_stride >= 0 && staging_bytes >= 0, "pccx_ply_load_host: negative size");
    if (B == 0) return PCCX_OK;
    PCCX_CHECK_ARG(paths && path_off && table && staging_host && dst_off && (msgs || msg_stride == 0), "pccx_ply_load_host: null pointer");
    PCCX_CHECK_ARG((uintptr_t)staging_host % 16 == 0, "pccx_ply_load_host: the staging buffer must be 16-byte aligned");
    Pool::get().run(B, threads > 0 ? threads : default_threads(), [&](int b) {
        int64_t *row = table + (size_t)b * PCCX_PLY_ROW;
        if (row[0] != PLY_OK) return;                  // refused by the scan: its status and message stay
        ply_load_one(paths + path_off[b], row, (uint8_t *)staging_host, staging_bytes, dst_off[b], msgs ? msgs + (size_t)b * msg_stride : nullptr, msg_stride);
    });
    return PCCX_OK;
}

extern "C" int pccx_ply_write_host(const float *rows_host, int64_t rows, const int64_t *first_row, const int64_t *count, int B, const char *dir,
                                   const char *names, const int64_t *name_off, const char *suffix, int threads)
{
    PCCX_CHECK_ARG(B >= 0 && rows >= 0, "pccx_ply_write_host: negative size");
    if (B == 0) return PCCX_OK;
    PCCX_CHECK_ARG(rows_host && first_row && count && dir && names && name_off && suffix, "pccx_ply_write_host: null pointer");
    for (int b = 0; b < B; ++b)                        // refused before touching the file system
        PCCX_CHECK_ARG(first_row[b] >= 0 && count[b] >= 0 && first_row[b] <= rows && count[b] <= rows - first_row[b],
                       "pccx_ply_write_host: cloud %d takes rows %lld .. +%lld of %lld", b, (long long)first_row[b], (long long)count[b], (long long)rows);
    const Names nm{dir, names, name_off};
    std::mutex emu;
    std::string first;
    int first_b = B;                                   // the error reported is the lowest cloud's, not the first in time: the same message
                                                       // whatever the threads' order
    Pool::get().run(B, threads > 0 ? threads : default_threads(), [&](int b) {
        // plyio.save_point_cloud's bytes: its four header lines, then little-endian float32 rows
        char head[160];
        const int hl = snprintf(head, sizeof(head), "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\n"
                                "property float z\nend_header\n", (long long)count[b]);
        std::string err;
        if (!write_all(nm.path(b, suffix).c_str(), rows_host + 3 * (size_t)first_row[b], 12 * (size_t)count[b], err, head, (size_t)hl)) {
            std::lock_guard<std::mutex> g(emu);
            if (b < first_b) first_b = b, first = err;
        }
    });
    if (first_b < B) {
        pccx_set_error("pccx_ply_write_host: %s", first.c_str());
        return PCCX_ERR_ARG;
    }
    return PCCX_OK;
}

// ---- OFF meshes on the same threads ("meshes"): scan the headers of a batch into a table, parse every body into
// one staging buffer.  A row of the table is PCCX_OFF_ROW int64: status (off_host.h OffStatus), nv, nf, byte offset of the body, file
// size, ne.  As for PLY files, a file that fails keeps its status in the row and its cause in msgs; the others are still done
// (ply_row_fail and pread_all above serve both formats).
namespace {

void off_scan_one(const char *path, int64_t *row, char *msg, int msg_stride)
{
    for (int j = 0; j < PCCX_OFF_ROW; ++j) row[j] = 0;
    if (msg && msg_stride > 0) msg[0] = 0;
    int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return ply_row_fail(row, msg, msg_stride, OFF_IO, std::string("open: ") + strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
        close(fd);
        return ply_row_fail(row, msg, msg_stride, OFF_IO, "not a regular file");
    }
    const int64_t size = (int64_t)st.st_size;
    row[4] = size;
    std::vector<uint8_t> buf;
    OffHeader h;
    char text[160];
    int status = OFF_TRUNCATED;
    // the header is the first lines with a token; comments in front of it may push it behind the 4 KiB read first
    for (int64_t want = 4096; status == OFF_TRUNCATED; want *= 4) {
        const size_t len = (size_t)(want < size ? want : size);
        buf.resize(len);
        std::string err;
        if (len && !pread_all(fd, buf.data(), len, 0, err)) {
            close(fd);
            return ply_row_fail(row, msg, msg_stride, OFF_IO, err);
        }
        status = off_parse_header(buf.data(), len, size, &h, text, sizeof(text));
        if ((int64_t)len >= size || want >= (16ll << 20)) break;
    }
    close(fd);
    if (status != OFF_OK) return ply_row_fail(row, msg, msg_stride, status, text);
    row[0] = OFF_OK, row[1] = h.nv, row[2] = h.nf, row[3] = h.body_offset, row[5] = h.ne;
}

void off_load_one(const char *path, int64_t *row, uint8_t *staging, int64_t staging_bytes, int64_t vdst, int64_t fdst, char *msg, int msg_stride)
{
    OffHeader h;
    h.nv = row[1], h.nf = row[2], h.body_offset = row[3], h.ne = row[5];
    const int64_t size = row[4];
    // the row is the caller's memory: nothing in it is trusted further than the scan's own limits
    if (h.nv < 3 || h.nv > OFF_MAX_VERTICES || h.nf < 1 || h.nf > OFF_MAX_FACES || h.body_offset < 0 || size < h.body_offset)
        return ply_row_fail(row, msg, msg_stride, OFF_ARG, "a table row that pccx_off_scan_host did not fill");
    const int64_t vb = 12 * h.nv, fb = 12 * h.nf;
    if (vdst < 0 || vdst % 4 != 0 || vdst > staging_bytes || vb > staging_bytes - vdst || fdst < 0 || fdst % 4 != 0 || fdst > staging_bytes ||
        fb > staging_bytes - fdst || (vdst < fdst + fb && fdst < vdst + vb))
        return ply_row_fail(row, msg, msg_stride, OFF_ARG, "the staging ranges of this file are not 4-byte aligned, overlap or do not hold its " +
                                                               std::to_string(vb) + " + " + std::to_string(fb) + " bytes");
    int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return ply_row_fail(row, msg, msg_stride, OFF_IO, std::string("open: ") + strerror(errno));
    std::string err;
    std::vector<uint8_t> text((size_t)(size - h.body_offset));
    const bool ok = text.empty() || pread_all(fd, text.data(), text.size(), h.body_offset, err);
    close(fd);
    if (!ok) return ply_row_fail(row, msg, msg_stride, OFF_IO, "the body could not be read as scanned (" + err + ")");
    char why[160];
    const int status = off_parse_body(text.data(), text.size(), h, (float *)(staging + vdst), (int32_t *)(staging + fdst), why, sizeof(why));
    if (status != OFF_OK) return ply_row_fail(row, msg, msg_stride, status, why);
}

}  // namespace

extern "C" int pccx_off_scan_host(int B, const char *paths, const int64_t *path_off, int64_t *table, char *msgs, int msg_stride, int threads)
{
    PCCX_CHECK_ARG(B >= 0 && msg_stride >= 0, "pccx_off_scan_host: negative size");
    if (B == 0) return PCCX_OK;
    PCCX_CHECK_ARG(paths && path_off && table && (msgs || msg_stride == 0), "pccx_off_scan_host: null pointer");
    Pool::get().run(B, threads > 0 ? threads : default_threads(), [&](int b) {
        off_scan_one(paths + path_off[b], table + (size_t)b * PCCX_OFF_ROW, msgs ? msgs + (size_t)b * msg_stride : nullptr, msg_stride);
    });
    return PCCX_OK;
}

extern "C" int pccx_off_load_host(int B, const char *paths, const int64_t *path_off, int64_t *table, void *staging_host, int64_t staging_bytes,
                                  const int64_t *v_dst_off, const int64_t *f_dst_off, char *msgs, int msg_stride, int threads)
{
    PCCX_CHECK_ARG(B >= 0 && msg_stride >= 0 && staging_bytes >= 0, "pccx_off_load_host: negative size");
    if (B == 0) return PCCX_OK;
    PCCX_CHECK_ARG(paths && path_off && table && staging_host && v_dst_off && f_dst_off && (msgs || msg_stride == 0), "pccx_off_load_host: null pointer");
    PCCX_CHECK_ARG((uintptr_t)staging_host % 4 == 0, "pccx_off_load_host: the staging buffer must be 4-byte aligned");
    Pool::get().run(B, threads > 0 ? threads : default_threads(), [&](int b) {
        int64_t *row = table + (size_t)b * PCCX_OFF_ROW;
        if (row[0] != OFF_OK) return;                  // refused by the scan: its status and message stay
        off_load_one(paths + path_off[b], row, (uint8_t *)staging_host, staging_bytes, v_dst_off[b], f_dst_off[b], msgs ? msgs + (size_t)b * msg_stride : nullptr,
                     msg_stride);
    });
    return PCCX_OK;
}

extern "C" size_t pccx_streams_packed_bytes(int B, int s_stride, int p_cap)
{
    if (B < 0 || s_stride < 0 || p_cap < 0) return 0;
    return Layout(B, s_stride, p_cap).end;
}
