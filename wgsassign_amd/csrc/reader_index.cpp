// The index of the streamed reader: ONE inflate pass that counts the sites of a Beagle file and records access points
// (serial for plain gzip; for BGZF in parallel, over threads and over the ranks of a node), the index and part files,
// and the entry points that build, merge and query them.  Host code only.
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>

#include "reader_impl.h"

namespace {

// Line bookkeeping of the index pass over consecutive pieces of output: non-blank lines completed, whether
// the line in progress has content, optional capture of every data line's first token (the site name).
struct LineScan {
    int64_t lines = 0;          // non-blank lines completed (the header is line 0)
    bool content = false, at_line_start = true, in_name = false, name_done = false;
    std::string header, *names = nullptr;
    bool header_done = false;

    void feed(const unsigned char *p, size_t n)
    {
        const unsigned char *e = p + n;
        while (p < e) {
            if (!header_done) {                      // keep the header line verbatim
                const unsigned char *nl = (const unsigned char *)memchr(p, '\n', (size_t)(e - p));
                header.append((const char *)p, (size_t)((nl ? nl : e) - p));
                if (!nl) return;
                header_done = true;
                lines += 1;                          // the header counts as a line even when empty
                content = false;
                at_line_start = true;
                p = nl + 1;
                continue;
            }
            if (!content) {                          // look for the first non-delimiter of the line
                while (p < e && *p != '\n' && is_delim((char)*p)) ++p, at_line_start = false;
                if (p == e) return;
                if (*p == '\n') {                    // blank line: not counted
                    at_line_start = true;
                    ++p;
                    continue;
                }
                content = true;
                at_line_start = false;
                in_name = names != nullptr;
                name_done = false;
            }
            if (in_name) {
                const unsigned char *t = p;
                while (t < e && !is_delim((char)*t)) ++t;
                names->append((const char *)p, (size_t)(t - p));
                p = t;
                if (p == e) return;
                names->push_back('\n');
                in_name = false;
            }
            const unsigned char *nl = (const unsigned char *)memchr(p, '\n', (size_t)(e - p));
            if (!nl) return;
            lines += 1;
            content = false;
            at_line_start = true;
            p = nl + 1;
        }
    }
    void finish()
    {
        if (!header_done) {
            header_done = true;
            lines += 1;
        } else if (content) {
            if (in_name) names->push_back('\n');
            lines += 1;                              // last line without a newline
        }
        content = false;
    }
};

// size and modification time in NANOSECONDS: a same-size rewrite within one second must not reuse a stale index
bool file_identity(const char *path, uint64_t &size, uint64_t &mtime)
{
    struct stat st;
    if (stat(path, &st) != 0) return false;
    size = (uint64_t)st.st_size;
    mtime = (uint64_t)st.st_mtim.tv_sec * 1000000000ull + (uint64_t)st.st_mtim.tv_nsec;
    return true;
}

// Cache files (index, site names) are written under a fresh name that must not exist (no symlink is followed, nothing
// of another user is overwritten) and renamed into place; they are read only if they are regular files of this user.
FILE *create_private(const std::string &final_path, std::string &tmp)
{
    for (int attempt = 0; attempt < 16; ++attempt) {
        tmp = final_path + ".tmp." + std::to_string((long)getpid()) + "." + std::to_string(attempt);
        const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
        if (fd >= 0) {
            FILE *f = fdopen(fd, "wb");
            if (!f) close(fd);
            return f;
        }
        if (errno != EEXIST) return nullptr;
    }
    return nullptr;
}

FILE *open_private(const char *path)
{
    const int fd = open(path, O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
    if (fd < 0) return nullptr;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_uid != geteuid()) {
        close(fd);
        return nullptr;
    }
    FILE *f = fdopen(fd, "rb");
    if (!f) close(fd);
    return f;
}

// One inflate pass: count the sites, read the header, record access points every `span` output bytes.
int scan_file(const char *path, int64_t span, BeagleIndex &idx, std::string *names)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) {
        wgs_set_error("cannot open Beagle file %s", path);
        return 2;
    }
    file_identity(path, idx.file_size, idx.mtime);
    // Output goes into 1 MiB laps of a buffer whose first GZ_WIN bytes always hold the 32 KiB that precede the lap
    // (copied there when a lap starts), so the dictionary of an access point is the GZ_WIN bytes before next_out,
    // contiguous -- and inflate is called per megabyte or deflate block, not per 32 KiB.
    constexpr size_t LAP = 1u << 20;
    std::vector<unsigned char> in(4u << 20), win(GZ_WIN + LAP);
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 15 + 32) != Z_OK) {
        fclose(fp);
        wgs_set_error("zlib initialisation failed");
        return 1;
    }
    LineScan ls;
    ls.names = names;
    uint64_t totin = 0, totout = 0, last = 0;
    bool member_start = true, bad = false;
    z.avail_out = 0;
    auto add_point = [&](bool at_member) {
        AccessPoint ap;
        ap.in = totin;
        ap.out = totout;
        ap.lines_before = ls.lines;
        ap.content = ls.content;
        ap.at_line_start = ls.at_line_start;
        ap.member_start = at_member;
        ap.bits = at_member ? 0 : (uint8_t)(z.data_type & 7);
        if (!at_member) ap.window.assign(z.next_out - GZ_WIN, z.next_out);       // the GZ_WIN bytes before `out`
        idx.points.push_back(std::move(ap));
        last = totout;
    };
    for (;;) {
        if (z.avail_in == 0) {
            const size_t got = fread(in.data(), 1, in.size(), fp);
            if (got == 0) break;
            z.next_in = in.data();
            z.avail_in = (unsigned)got;
        }
        if (member_start && span > 0 && totout - last >= (uint64_t)span && totout > 0) add_point(true);
        member_start = false;
        if (z.avail_out == 0) {                      // new lap: keep the last GZ_WIN bytes in front of it
            if (totout > 0) memmove(win.data(), z.next_out - GZ_WIN, GZ_WIN);
            z.avail_out = (unsigned)LAP;
            z.next_out = win.data() + GZ_WIN;
        }
        const unsigned char *produced_at = z.next_out;
        const unsigned in0 = z.avail_in, out0 = z.avail_out;
        const int ret = inflate(&z, Z_BLOCK);
        totin += in0 - z.avail_in;
        totout += out0 - z.avail_out;
        ls.feed(produced_at, out0 - z.avail_out);
        if (ret == Z_STREAM_END) {                   // next gzip member, if any
            if (z.avail_in == 0) {
                const size_t got = fread(in.data(), 1, in.size(), fp);
                z.next_in = in.data();
                z.avail_in = (unsigned)got;
                if (got == 0) break;
            }
            if (inflateReset2(&z, 15 + 32) != Z_OK) {
                bad = true;
                break;
            }
            member_start = true;
            continue;
        }
        if (ret != Z_OK && ret != Z_BUF_ERROR) {
            bad = true;
            break;
        }
        // at the end of a deflate block that is not the last of its member
        if (span > 0 && (z.data_type & 128) && !(z.data_type & 64) && totout - last >= (uint64_t)span && totout >= GZ_WIN)
            add_point(false);
    }
    inflateEnd(&z);
    fclose(fp);
    if (bad) {
        wgs_set_error("read error in %s (corrupt gzip stream)", path);
        return 1;
    }
    ls.finish();
    idx.sites = ls.lines > 0 ? ls.lines - 1 : 0;     // minus the header line
    parse_header(ls.header.data(), ls.header.data() + ls.header.size(), idx.samples, idx.gl_cols);
    return 0;
}

// ---- the same pass for BGZF files, in parallel -----------------------------------------------------------------
// The block table (offsets, compressed and uncompressed sizes) comes from hopping over the member headers and
// trailers -- nothing is inflated for it.  Worker threads then inflate disjoint ranges of blocks and summarise each:
// where its first newline is, whether there is text before it, how many non-blank lines end after it, and what is
// left open at its end.  A serial pass over the summaries (a few words per 64 KiB of input) turns them into global
// line numbers; access points are block starts (no dictionaries).
struct BlockLines {
    uint8_t has_nl = 0;             // the block contains a newline
    uint8_t content_before = 0;     // non-delimiter text before the first newline (or anywhere, if there is none)
    uint8_t content_after = 0;      // non-delimiter text after the last newline
    uint8_t last_is_nl = 0;         // the block ends with a newline
    int32_t lines_after_first = 0;  // non-blank lines that start AND end inside the block
};

bool bgzf_block_table(const char *path, std::vector<BgzfBlock> &blocks)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) return false;
    Bgzf k;
    for (uint64_t off = 0;; off += blocks.back().csize) {
        BgzfBlock b;
        if ((k = bgzf_member_at(fileno(fp), off, 512, UINT64_MAX, b)) != Bgzf::member) break;
        blocks.push_back(b);
    }
    fclose(fp);
    return k == Bgzf::need_more && !blocks.empty();          // the hops ended with the file
}

void summarise_block(const unsigned char *p, size_t n, BlockLines &bl)
{
    const unsigned char *e = p + n;
    const unsigned char *nl = (const unsigned char *)memchr(p, '\n', n);
    const unsigned char *seg_end = nl ? nl : e;
    for (const unsigned char *t = p; t < seg_end && !bl.content_before; ++t) bl.content_before = !is_delim((char)*t);
    if (!nl) return;
    bl.has_nl = 1;
    const unsigned char *q = nl + 1;
    for (;;) {
        const unsigned char *nx = (const unsigned char *)memchr(q, '\n', (size_t)(e - q));
        const unsigned char *end = nx ? nx : e;
        bool content = false;
        for (const unsigned char *t = q; t < end && !content; ++t) content = !is_delim((char)*t);
        if (!nx) {
            bl.content_after = content;
            break;
        }
        bl.lines_after_first += content;
        q = nx + 1;
    }
    bl.last_is_nl = n > 0 && p[n - 1] == '\n';
}

// ---- the BGZF pass in parts: threads of one process, and processes of one node -------------------------------------
// Finding the blocks by hopping from header to header is serial (41 M hops for 2.7 TB of text), and so was the pass of
// round 2 across ranks (the first rank inflated the whole file).  A part -- any byte range of the file -- can find its own
// first block instead: BGZF members start with a 16-byte signature (gzip magic, FEXTRA, XLEN = 6, 'B' 'C' 2 0); the first
// position at or after the range's start where a header parses AND three further hops land on headers (or the end of the
// file) is taken as a block boundary.  That is a heuristic only for SPEED: every part reports where it started and where
// the block after its last one starts, and the merge accepts the parts only if they chain exactly (part 0 starts at byte
// 0, so by induction every part hopped the true chain); otherwise the classic serial hop takes over.
struct PartData {
    uint64_t first = 0, next = 0;          // file offset of the part's first block / of the first block after its last
    std::vector<BgzfBlock> blocks;
    std::vector<BlockLines> sum;
    std::string header;                    // part 0: the header line
    bool header_done = false;
};

// Parses the member at file offset `off`: 1 = a BGZF block, 0 = end of file exactly at off, -1 = anything else.
int bgzf_block_at(int fd, uint64_t file_size, uint64_t off, BgzfBlock &b)
{
    if (off == file_size) return 0;
    return bgzf_member_at(fd, off, 64, file_size, b) == Bgzf::member ? 1 : -1;
}

// First block boundary at or after `from` (from > 0): see above.  Returns file_size when the rest holds no block start.
uint64_t bgzf_resync(int fd, uint64_t file_size, uint64_t from)
{
    std::vector<unsigned char> win(1u << 20);
    for (uint64_t base = from; base < file_size;) {
        const ssize_t got = pread(fd, win.data(), win.size(), (off_t)base);
        if (got < 16) return file_size;
        for (ssize_t i = 0; i + 16 <= got; ++i) {
            const unsigned char *q = win.data() + i;
            if (q[0] != 31 || q[1] != 139 || q[2] != 8 || q[3] != 4) continue;
            uint64_t at = base + (uint64_t)i;
            bool chain = true;
            for (int hop = 0; hop < 4 && chain; ++hop) {
                BgzfBlock b;
                const int k = bgzf_block_at(fd, file_size, at, b);
                if (k == 0) break;                            // the chain ends with the file: fine
                chain = k > 0;
                at += b.csize;
            }
            if (chain) return base + (uint64_t)i;
        }
        base += (uint64_t)got - 15;                           // a signature may straddle the window's end
    }
    return file_size;
}

// The blocks that START in [lo, hi), inflated and summarised: one thread's share.
bool bgzf_part_thread(const char *path, uint64_t file_size, uint64_t lo, uint64_t hi, bool want_header, PartData &out)
{
    FILE *fp = fopen(path, "rb");
    BlockInflater inf;
    if (!fp || !inf.init()) {
        if (fp) fclose(fp);
        return false;
    }
    const int fd = fileno(fp);
    uint64_t at = lo == 0 ? 0 : bgzf_resync(fd, file_size, lo);
    out.first = at;
    std::vector<unsigned char> cb(65536 + 4096), ob(65536);
    bool ok = true;
    while (at < hi && at < file_size) {
        BgzfBlock b;
        if (bgzf_block_at(fd, file_size, at, b) <= 0 || !inf.run_at(fd, b, cb.data(), ob.data())) {
            ok = false;
            break;
        }
        BlockLines bl;
        summarise_block(ob.data(), b.isize, bl);
        if (want_header && !out.header_done && b.isize > 0) {
            const unsigned char *nl = (const unsigned char *)memchr(ob.data(), '\n', b.isize);
            out.header.append((const char *)ob.data(), nl ? (size_t)(nl - ob.data()) : b.isize);
            out.header_done = nl != nullptr;
        }
        out.blocks.push_back(b);
        out.sum.push_back(bl);
        at += b.csize;
    }
    out.next = at;
    fclose(fp);
    return ok;
}

// Part `part` of `nparts` (equal byte ranges of the file) on `threads` threads.  0 = ok, -1 = not BGZF / the sub-ranges
// did not chain (the caller falls back to the serial hop), 1 = read error.
int bgzf_collect_part(const char *path, int part, int nparts, int threads, PartData &out)
{
    uint64_t file_size = 0, mtime = 0;
    if (!file_identity(path, file_size, mtime)) return 1;
    {
        FILE *fp = fopen(path, "rb");
        if (!fp) return 1;
        BgzfBlock b;
        const int k = bgzf_block_at(fileno(fp), file_size, 0, b);
        fclose(fp);
        if (k <= 0) return -1;
    }
    const uint64_t lo = file_size * (uint64_t)part / (uint64_t)nparts, hi = file_size * (uint64_t)(part + 1) / (uint64_t)nparts;
    const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)(threads > 0 ? threads : 1), (hi - lo) >> 20));
    std::vector<PartData> sub(T);
    std::vector<char> ok(T, 1);
    run_threads(T, [&](int t) {
        const uint64_t a = lo + (hi - lo) * (uint64_t)t / (uint64_t)T, b = lo + (hi - lo) * (uint64_t)(t + 1) / (uint64_t)T;
        ok[t] = bgzf_part_thread(path, file_size, a, b, part == 0 && t == 0, sub[t]);
    });
    for (char c : ok)
        if (!c) return -1;
    out = PartData();
    out.first = sub[0].first;
    for (int t = 0; t < T; ++t) {
        if (t > 0 && sub[t].first != sub[t - 1].next) return -1;          // a sub-range started off the chain
        out.blocks.insert(out.blocks.end(), sub[t].blocks.begin(), sub[t].blocks.end());
        out.sum.insert(out.sum.end(), sub[t].sum.begin(), sub[t].sum.end());
    }
    out.next = sub[T - 1].next;
    out.header = sub[0].header;
    out.header_done = sub[0].header_done;
    // a header line longer than the first thread's share: finish it serially
    if (part == 0 && !out.header_done) {
        out.header.clear();
        FILE *fp = fopen(path, "rb");
        BlockInflater inf;
        if (!fp || !inf.init()) {
            if (fp) fclose(fp);
            return 1;
        }
        std::vector<unsigned char> cb(65536 + 4096), ob(65536);
        for (const BgzfBlock &b : out.blocks) {
            if (!inf.run_at(fileno(fp), b, cb.data(), ob.data())) break;
            const unsigned char *nl = (const unsigned char *)memchr(ob.data(), '\n', b.isize);
            out.header.append((const char *)ob.data(), nl ? (size_t)(nl - ob.data()) : b.isize);
            if (nl) break;
        }
        fclose(fp);
    }
    return 0;
}

// The serial pass over the block summaries of all parts, in file order: line numbers at every block start, access points.
// -1 when the parts do not chain.
int bgzf_merge_parts(const char *path, const std::vector<PartData> &parts, int64_t span, BeagleIndex &idx)
{
    uint64_t file_size = 0;
    if (!file_identity(path, idx.file_size, idx.mtime)) return 1;
    file_size = idx.file_size;
    uint64_t expect = 0;
    for (const PartData &p : parts) {
        if (p.first != expect) return -1;
        expect = p.next;
    }
    if (expect != file_size) return -1;
    int64_t lines = 0;              // non-blank lines completed
    bool content = false, at_line_start = true, header_done = false;
    uint64_t out = 0, last = 0;
    for (const PartData &p : parts) {
        for (size_t i = 0; i < p.blocks.size(); ++i) {
            const BgzfBlock &blk = p.blocks[i];
            const BlockLines &bl = p.sum[i];
            if (span > 0 && out > 0 && out - last >= (uint64_t)span && blk.isize > 0 && header_done) {
                AccessPoint ap;
                ap.in = blk.off;
                ap.out = out;
                ap.lines_before = lines;
                ap.content = content;
                ap.at_line_start = at_line_start;
                ap.member_start = 1;
                idx.points.push_back(std::move(ap));
                last = out;
            }
            if (blk.isize == 0) continue;
            if (bl.has_nl) {
                // the header counts as a line even when it is empty (LineScan); every other line only when non-blank
                lines += !header_done ? 1 : (content || bl.content_before);
                header_done = true;
                lines += bl.lines_after_first;
                content = bl.content_after;
                at_line_start = bl.last_is_nl;
            } else {
                content = content || bl.content_before;
                at_line_start = false;
            }
            out += blk.isize;
        }
    }
    if (!header_done) lines += 1;
    else if (content) lines += 1;   // last line without a newline
    idx.sites = lines > 0 ? lines - 1 : 0;
    const std::string &header = parts.empty() ? std::string() : parts[0].header;
    parse_header(header.data(), header.data() + header.size(), idx.samples, idx.gl_cols);
    return 0;
}

// Returns 0 on success, -1 when the file is not (entirely) BGZF -- the caller then takes the serial pass.
int scan_file_bgzf(const char *path, int64_t span, int threads, BeagleIndex &idx)
{
    std::vector<PartData> parts(1);
    int rc = bgzf_collect_part(path, 0, 1, threads, parts[0]);
    if (rc == 0) rc = bgzf_merge_parts(path, parts, span, idx);
    if (rc == -1) {
        // the sub-ranges did not chain (or this is not BGZF at all): the classic serial hop decides
        std::vector<BgzfBlock> blocks;
        if (!bgzf_block_table(path, blocks)) return -1;
        idx = BeagleIndex();
        parts.assign(1, PartData());
        uint64_t file_size = 0, mtime = 0;
        file_identity(path, file_size, mtime);
        parts[0].first = 0;
        if (!bgzf_part_thread(path, file_size, 0, file_size, true, parts[0])) {
            wgs_set_error("read error in %s (corrupt BGZF block)", path);
            return 1;
        }
        rc = bgzf_merge_parts(path, parts, span, idx);
    }
    if (rc == 1) wgs_set_error("read error in %s (corrupt BGZF block)", path);
    return rc;
}

template <typename T>
void put(FILE *f, const T &v) { fwrite(&v, sizeof v, 1, f); }
template <typename T>
bool get(FILE *f, T &v) { return fread(&v, sizeof v, 1, f) == 1; }

const char kIndexMagic[8] = {'W', 'G', 'S', 'I', 'D', 'X', '3', 0};     // 3: modification time in nanoseconds

bool save_index(const char *path, const BeagleIndex &idx)
{
    std::string tmp;
    FILE *f = create_private(path, tmp);
    if (!f) return false;
    fwrite(kIndexMagic, 1, 8, f);
    put(f, idx.file_size);
    put(f, idx.mtime);
    put(f, idx.sites);
    put(f, idx.gl_cols);
    const int32_t ns = (int32_t)idx.samples.size(), np = (int32_t)idx.points.size();
    put(f, ns);
    for (const auto &s : idx.samples) {
        const int32_t l = (int32_t)s.size();
        put(f, l);
        fwrite(s.data(), 1, s.size(), f);
    }
    put(f, np);
    for (const auto &a : idx.points) {
        put(f, a.in);
        put(f, a.out);
        put(f, a.lines_before);
        put(f, a.bits);
        put(f, a.content);
        put(f, a.at_line_start);
        put(f, a.member_start);
        if (!a.member_start) {                                // the 32 KiB dictionary, deflated (text: ~4x smaller)
            std::vector<unsigned char> z(compressBound(GZ_WIN));
            uLongf zn = (uLongf)z.size();
            if (compress2(z.data(), &zn, a.window.data(), GZ_WIN, 1) != Z_OK) {
                fclose(f);
                return false;
            }
            const uint32_t n32 = (uint32_t)zn;
            put(f, n32);
            fwrite(z.data(), 1, zn, f);
        }
    }
    const bool ok = !ferror(f) && fflush(f) == 0;
    fclose(f);
    if (ok && rename(tmp.c_str(), path) == 0) return true;     // atomic: readers never see a partial index
    unlink(tmp.c_str());
    return false;
}

bool load_index(const char *path, BeagleIndex &idx)
{
    FILE *f = open_private(path);
    if (!f) return false;
    char magic[8];
    bool ok = fread(magic, 1, 8, f) == 8 && memcmp(magic, kIndexMagic, 8) == 0;
    int32_t ns = 0, np = 0;
    ok = ok && get(f, idx.file_size) && get(f, idx.mtime) && get(f, idx.sites) && get(f, idx.gl_cols) && get(f, ns) && ns >= 0;
    for (int i = 0; ok && i < ns; ++i) {
        int32_t l = 0;
        ok = get(f, l) && l >= 0 && l < (1 << 20);
        if (!ok) break;
        std::string s((size_t)l, '\0');
        ok = fread(&s[0], 1, (size_t)l, f) == (size_t)l;
        idx.samples.push_back(std::move(s));
    }
    ok = ok && get(f, np) && np >= 0;
    for (int i = 0; ok && i < np; ++i) {
        AccessPoint a;
        ok = get(f, a.in) && get(f, a.out) && get(f, a.lines_before) && get(f, a.bits) && get(f, a.content) &&
             get(f, a.at_line_start) && get(f, a.member_start);
        if (ok && !a.member_start) {
            uint32_t zn = 0;
            ok = get(f, zn) && zn > 0 && zn <= compressBound(GZ_WIN);
            std::vector<unsigned char> z(ok ? zn : 0);
            ok = ok && fread(z.data(), 1, zn, f) == zn;
            a.window.resize(GZ_WIN);
            uLongf out = GZ_WIN;
            ok = ok && uncompress(a.window.data(), &out, z.data(), zn) == Z_OK && out == GZ_WIN;
        }
        if (ok) idx.points.push_back(std::move(a));
    }
    fclose(f);
    return ok;
}

// at most max_points access points (0: all of them), thinned out evenly
void thin_points(BeagleIndex &idx, int32_t max_points)
{
    if (max_points <= 0 || (int64_t)idx.points.size() <= max_points) return;
    std::vector<AccessPoint> keep;
    const double step = (double)idx.points.size() / max_points;
    for (int i = 0; i < max_points; ++i) keep.push_back(std::move(idx.points[(size_t)(i * step)]));
    idx.points.swap(keep);
}

const char kPartMagic[8] = {'W', 'G', 'S', 'P', 'R', 'T', '1', 0};

bool save_part(const char *path_out, const PartData &p, uint64_t file_size, uint64_t mtime)
{
    std::string tmp;
    FILE *f = create_private(path_out, tmp);
    if (!f) return false;
    fwrite(kPartMagic, 1, 8, f);
    put(f, file_size);
    put(f, mtime);
    put(f, p.first);
    put(f, p.next);
    const uint64_t nb = p.blocks.size(), hl = p.header.size();
    put(f, nb);
    put(f, hl);
    fwrite(p.header.data(), 1, p.header.size(), f);
    if (nb) {
        fwrite(p.blocks.data(), sizeof(BgzfBlock), nb, f);
        fwrite(p.sum.data(), sizeof(BlockLines), nb, f);
    }
    const bool ok = !ferror(f) && fflush(f) == 0;
    fclose(f);
    if (ok && rename(tmp.c_str(), path_out) == 0) return true;
    unlink(tmp.c_str());
    return false;
}

bool load_part(const char *path_in, PartData &p, uint64_t file_size, uint64_t mtime)
{
    FILE *f = open_private(path_in);
    if (!f) return false;
    char magic[8];
    uint64_t fs = 0, mt = 0, nb = 0, hl = 0;
    bool ok = fread(magic, 1, 8, f) == 8 && memcmp(magic, kPartMagic, 8) == 0 && get(f, fs) && get(f, mt) && get(f, p.first) && get(f, p.next) &&
              get(f, nb) && get(f, hl) && fs == file_size && mt == mtime && hl < (1u << 30) && nb < (1ull << 40);
    if (ok) {
        // the counts must fit the part file itself BEFORE anything is sized by them: a damaged part file would otherwise ask for
        // terabytes (std::bad_alloc through an extern "C" entry point)
        struct stat sb;
        const uint64_t fixed = 8 + 6 * sizeof(uint64_t);
        ok = fstat(fileno(f), &sb) == 0 && (uint64_t)sb.st_size >= fixed && hl <= (uint64_t)sb.st_size - fixed &&
             nb <= ((uint64_t)sb.st_size - fixed - hl) / (sizeof(BgzfBlock) + sizeof(BlockLines));
    }
    if (ok) {
        p.header.resize((size_t)hl);
        ok = fread(&p.header[0], 1, (size_t)hl, f) == (size_t)hl || hl == 0;
        p.blocks.resize((size_t)nb);
        p.sum.resize((size_t)nb);
        if (ok && nb) ok = fread(p.blocks.data(), sizeof(BgzfBlock), (size_t)nb, f) == (size_t)nb && fread(p.sum.data(), sizeof(BlockLines), (size_t)nb, f) == (size_t)nb;
    }
    fclose(f);
    return ok;
}

}  // namespace

bool index_matches_file(const char *index_path, const char *path, BeagleIndex &idx)
{
    uint64_t size = 0, mtime = 0;
    return load_index(index_path, idx) && file_identity(path, size, mtime) && size == idx.file_size && mtime == idx.mtime;
}

extern "C" {

/* ONE inflate pass over a gzipped Beagle file: counts its sites, and (index_path != NULL) writes an index --
 * header fields plus at most max_points access points, about `span_bytes` of text apart -- from which
 * wgs_reader_open_indexed starts at any row without inflating what precedes it; names_path != NULL also
 * receives every site name, '\n'-terminated (the names-only pass of the downsampled-LOO site masks). */
int wgs_reader_build_index(const char *path, const char *index_path, const char *names_path, int64_t span_bytes, int32_t max_points,
                           int64_t *sites)
{
    if (!path || !sites) {
        wgs_set_error("null argument");
        return 2;
    }
    BeagleIndex idx;
    std::string names;
    const int64_t span = index_path ? std::max<int64_t>(span_bytes, (int64_t)GZ_WIN) : 0;
    // BGZF input (what ANGSD writes): blocks are independent -> all host threads.  Site names then come from a second
    // pass whose blocks are inflated in parallel as well (GzSource::read_bgzf) and only scanned serially for the first
    // token of every line -- a memchr per line.  Anything else: one serial inflate pass that does everything.
    const int threads = (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 32u);
    int rc = scan_file_bgzf(path, span, threads, idx);
    if (rc == 0 && names_path) {
        GzSource src;
        if (!src.open(path, nullptr)) {
            wgs_set_error("cannot open Beagle file %s", path);
            return 2;
        }
        src.try_bgzf(threads);
        LineScan ls;
        ls.names = &names;
        std::vector<char> buf(64u << 20);
        for (;;) {
            const long got = src.read(buf.data(), buf.size());
            if (got < 0) {
                wgs_set_error("read error in %s (corrupt gzip stream)", path);
                return 1;
            }
            if (got == 0) break;
            ls.feed(reinterpret_cast<const unsigned char *>(buf.data()), (size_t)got);
        }
        ls.finish();
        if ((ls.lines > 0 ? ls.lines - 1 : 0) != idx.sites) {
            wgs_set_error("Beagle file %s: the two passes disagree about the number of sites", path);
            return 1;
        }
    }
    if (rc < 0) {
        idx = BeagleIndex();
        rc = scan_file(path, span, idx, names_path ? &names : nullptr);
    }
    if (rc) return rc;
    *sites = idx.sites;
    // the site names first, then the index: an index in place implies that the names written with it are complete
    // (both appear by rename; a run that is killed in between leaves a names file without an index -- rebuilt)
    if (names_path) {
        std::string tmp;
        FILE *f = create_private(names_path, tmp);
        const bool ok = f && fwrite(names.data(), 1, names.size(), f) == names.size() && fflush(f) == 0;
        if (f) fclose(f);
        if (!ok || rename(tmp.c_str(), names_path) != 0) {
            if (f) unlink(tmp.c_str());
            wgs_set_error("cannot write the site names to %s", names_path);
            return 1;
        }
    }
    if (index_path) {
        thin_points(idx, max_points);
        if (!save_index(index_path, idx)) {
            wgs_set_error("cannot write the Beagle index %s", index_path);
            return 1;
        }
    }
    return 0;
}

/* The index pass of a BGZF file split over the ranks of a node: rank `part` of `nparts` inflates and summarises the blocks
 * of its byte range (on `threads` threads) into part_path; wgs_reader_index_merge (one rank, after a barrier) chains the
 * parts into the index.  rc 3 = this file cannot be done in parts (not BGZF, or a range did not find the block chain): one
 * rank then calls wgs_reader_build_index as before. */
int wgs_reader_index_part(const char *path, const char *part_path, int part, int nparts, int threads)
{
    if (!path || !part_path || part < 0 || nparts < 1 || part >= nparts) {
        wgs_set_error("bad argument");
        return 2;
    }
    PartData p;
    const int rc = bgzf_collect_part(path, part, nparts, threads, p);
    if (rc == -1) {
        wgs_set_error("%s cannot be indexed in parts", path);
        return 3;
    }
    if (rc) {
        wgs_set_error("read error in %s (corrupt BGZF block)", path);
        return 1;
    }
    uint64_t size = 0, mtime = 0;
    file_identity(path, size, mtime);
    if (!save_part(part_path, p, size, mtime)) {
        wgs_set_error("cannot write %s", part_path);
        return 1;
    }
    return 0;
}

int wgs_reader_index_merge(const char *path, const char *index_path, const char *parts_prefix, int nparts, int64_t span_bytes,
                           int32_t max_points, int64_t *sites)
{
    if (!path || !index_path || !parts_prefix || nparts < 1 || !sites) {
        wgs_set_error("bad argument");
        return 2;
    }
    uint64_t size = 0, mtime = 0;
    if (!file_identity(path, size, mtime)) {
        wgs_set_error("cannot open Beagle file %s", path);
        return 2;
    }
    // the part files are this call's to remove, however it ends (the caller falls back to the one-rank pass on rc 3)
    struct PartFiles {
        std::string prefix;
        int n;
        ~PartFiles() { for (int k = 0; k < n; ++k) unlink((prefix + "." + std::to_string(k)).c_str()); }
    } cleanup{std::string(parts_prefix), nparts};
    std::vector<PartData> parts((size_t)nparts);
    for (int k = 0; k < nparts; ++k) {
        const std::string pp = std::string(parts_prefix) + "." + std::to_string(k);
        if (!load_part(pp.c_str(), parts[(size_t)k], size, mtime)) {
            wgs_set_error("%s is not a part of the index of %s", pp.c_str(), path);
            return 3;
        }
    }
    BeagleIndex idx;
    const int rc = bgzf_merge_parts(path, parts, std::max<int64_t>(span_bytes, (int64_t)GZ_WIN), idx);
    if (rc == -1) {
        wgs_set_error("the parts of the index of %s do not chain", path);
        return 3;
    }
    if (rc) {
        wgs_set_error("read error in %s", path);
        return 1;
    }
    thin_points(idx, max_points);
    if (!save_index(index_path, idx)) {
        wgs_set_error("cannot write the Beagle index %s", index_path);
        return 1;
    }
    *sites = idx.sites;
    return 0;
}

/* Sites of the file an index was built for (after checking that it still describes `path`: size and mtime). */
int wgs_reader_index_sites(const char *path, const char *index_path, int64_t *sites)
{
    if (!path || !index_path || !sites) {
        wgs_set_error("null argument");
        return 2;
    }
    BeagleIndex idx;
    if (!index_matches_file(index_path, path, idx)) {
        wgs_set_error("%s is not an index of %s", index_path, path);
        return 2;
    }
    *sites = idx.sites;
    return 0;
}

int wgs_reader_count_sites(const char *path, int64_t *sites) { return wgs_reader_build_index(path, nullptr, nullptr, 0, 0, sites); }

/* About how many sites a BGZF file holds, from five samples of a quarter megabyte each (start, quartiles, end): the newlines of the
 * blocks that start there, per compressed byte, times the file's size.  Milliseconds instead of the index pass's inflate of
 * everything -- for the caller that wants to size a device matrix BEFORE it knows (stream_to_device's one-pass cold path: the exact
 * count arrives with the index, which is built meanwhile).  rc 3: not BGZF, or a sample fell off the block chain. */
int wgs_reader_estimate_sites(const char *path, int64_t *estimate)
{
    if (!path || !estimate) {
        wgs_set_error("null argument");
        return 2;
    }
    *estimate = 0;
    uint64_t file_size = 0, mtime = 0;
    if (!file_identity(path, file_size, mtime)) {
        wgs_set_error("cannot open Beagle file %s", path);
        return 2;
    }
    {
        FILE *fp = fopen(path, "rb");
        if (!fp) {
            wgs_set_error("cannot open Beagle file %s", path);
            return 2;
        }
        BgzfBlock b;
        const int k = bgzf_block_at(fileno(fp), file_size, 0, b);
        fclose(fp);
        if (k <= 0) return 3;
    }
    const uint64_t window = 256u << 10;
    double newlines = 0.0, comp = 0.0;
    for (int q = 0; q < 5; ++q) {
        uint64_t lo = q == 4 ? (file_size > window ? file_size - window : 0) : file_size / 4 * (uint64_t)q;
        if (q > 0 && lo < window) continue;                           // a file smaller than the samples: the first one is all of it
        PartData pd;
        if (!bgzf_part_thread(path, file_size, lo, std::min(file_size, lo + window), false, pd)) return 3;
        for (size_t i = 0; i < pd.blocks.size(); ++i) {
            newlines += (double)pd.sum[i].lines_after_first + (pd.sum[i].has_nl ? 1.0 : 0.0);
            comp += (double)pd.blocks[i].csize;
        }
    }
    if (comp <= 0.0) return 3;
    *estimate = (int64_t)(newlines / comp * (double)file_size);
    return 0;
}

}  // extern "C"
