// Trace of everything the streamed reader shows through the C ABI and csrc/reader_text.h, as deterministic text: no timings,
// no pointers, no absolute paths.  Run in a directory that holds copies of tests/golden/reader/*:
//     reader_trace FILE...        (bare names: beagle*.gz, table*, bad_*.gz; index, names and part files are written beside them)
// tests/test_reader_trace_cpu.py holds the output to tests/golden/reader_trace.txt, which was recorded from the reader before
// it was split into units.  Host code only; links every csrc/reader*.cpp and brings its own wgs_set_error.
#include <fcntl.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "reader_text.h"
#include "wgsassign_hip.h"
#include "wgsassign_hip_debug.h"

static char g_err[1024];
void wgs_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

namespace {

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(const void *p, size_t n)
    {
        const unsigned char *b = (const unsigned char *)p;
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    }
    template <typename T>
    void vec(const std::vector<T> &v) { add(v.data(), v.size() * sizeof(T)); }
};

// rc, and the message when there is one
void say_rc(const char *what, int rc)
{
    if (rc) printf("  %s: rc %d: %s\n", what, rc, g_err);
    else printf("  %s: rc 0\n", what);
}

// digest of a file's bytes from `skip` on
std::string file_digest(const std::string &path, size_t skip)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return "absent";
    std::vector<unsigned char> all;
    unsigned char buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
    fclose(f);
    Fnv h;
    if (all.size() > skip) h.add(all.data() + skip, all.size() - skip);
    char out[64];
    snprintf(out, sizeof out, "%zu bytes %016llx", all.size(), (unsigned long long)h.h);
    return out;
}

// Per-chunk lines: the first few are printed, the rest folded into one digest (the 700-byte members make thousands of chunks).
struct ChunkLog {
    int n = 0;
    Fnv rest;
    void line(const char *fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        if (n < 6) printf("    chunk %d: %s\n", n, buf);
        else rest.add(buf, strlen(buf) + 1);
        ++n;
    }
    void end()
    {
        if (n > 6) printf("    and %d more chunks: %016llx\n", n - 6, (unsigned long long)rest.h);
        else printf("    %d chunks\n", n);
    }
};

TextAllocator heap()
{
    TextAllocator a;
    a.alloc = [](size_t n, void *) { return malloc(n); };
    a.release = [](void *p, void *) { free(p); };
    return a;
}

// every row and site name the line-oriented calls still give
int read_all(wgs_reader *r, int64_t chunk, int64_t *rows_out, uint64_t *digest)
{
    const int n = wgs_reader_n_individuals(r);
    std::vector<float> buf((size_t)chunk * 2 * n + 1);
    Fnv h;
    *rows_out = 0;
    for (;;) {
        int64_t got = 0;
        if (int rc = wgs_reader_next(r, buf.data(), chunk, &got)) return rc;
        if (got == 0) break;
        h.add(buf.data(), (size_t)got * 2 * n * 4);
        int64_t nb = 0;
        const char *names = wgs_reader_chunk_sites(r, &nb);
        h.add(names, (size_t)nb);
        *rows_out += got;
    }
    *digest = h.h;
    return 0;
}

void trace_rows(const char *what, wgs_reader *r)
{
    int64_t rows = 0;
    uint64_t h = 0;
    const int rc = read_all(r, 777, &rows, &h);
    if (rc) printf("  %s: rc %d after %lld rows: %s\n", what, rc, (long long)rows, g_err);
    else printf("  %s: %lld rows %016llx\n", what, (long long)rows, (unsigned long long)h);
}

void trace_text(wgs_reader *r, int64_t limit)
{
    const int64_t before = reader_text_lines_read(r);
    int rc = reader_text_start(r, 1, 2, heap(), limit);
    if (rc) return say_rc("reader_text_start", rc);
    ChunkLog log;
    for (;;) {
        TextChunk *c = nullptr;
        double waited = 0.0;
        if ((rc = reader_text_next(r, &c, &waited)) != 0 || !c) break;
        Fnv lines, names, text;
        lines.vec(c->begin);
        lines.vec(c->end);
        lines.vec(c->lineno);
        names.add(c->names.data(), c->names.size());
        text.add(c->data, c->len);
        bool padded = c->cap >= c->len + TEXT_PAD;
        for (size_t i = 0; padded && i < TEXT_PAD; ++i) padded = c->data[c->len + i] == '\n';
        log.line("first_row %lld first_line %lld len %zu lines %zu offsets %016llx names %016llx text %016llx pad %d", (long long)c->first_row,
                 (long long)c->first_line, c->len, c->begin.size(), (unsigned long long)lines.h, (unsigned long long)names.h, (unsigned long long)text.h,
                 (int)padded);
        reader_text_release(r, c);
    }
    log.end();
    reader_text_stop(r);
    say_rc("reader_text_next at the end", rc);
    printf("    rows counted %lld, chunks %lld\n", (long long)(reader_text_lines_read(r) - before), (long long)wgs_debug_reader_text_chunks(r));
}

void trace_comp(wgs_reader *r, size_t max_members)
{
    printf("    bytes left before %lld\n", (long long)reader_comp_bytes_left(r));
    int rc = reader_comp_start(r, 1, 1, 2, heap(), max_members);
    if (rc) return say_rc("reader_comp_start", rc);
    ChunkLog log;
    for (;;) {
        CompChunk *c = nullptr;
        if ((rc = reader_comp_next(r, &c, nullptr)) != 0 || !c) break;
        Fnv lists, pre, text;
        lists.vec(c->in_off);
        lists.vec(c->in_len);
        lists.vec(c->isize);
        pre.add(c->pre_text, c->pre_len);
        std::vector<unsigned char> out(65536);
        bool inflated = true;
        for (size_t i = 0; i < c->isize.size(); ++i) {
            if (!reader_inflate_member(c->comp + c->in_off[i], c->in_len[i], c->isize[i], out.data())) inflated = false;
            else text.add(out.data(), c->isize[i]);
        }
        log.line("pre_len %zu pre %016llx len %zu text_bytes %zu last %d members %zu lists %016llx text %016llx inflated %d", c->pre_len,
                 (unsigned long long)pre.h, c->len, c->text_bytes, (int)c->last, c->isize.size(), (unsigned long long)lists.h, (unsigned long long)text.h,
                 (int)inflated);
        const bool last = c->last;
        reader_comp_release(r, c);
        if (last) break;
    }
    log.end();
    say_rc("reader_comp_next at the end", rc);
    reader_comp_stop(r);
    int64_t got = -1;
    std::vector<float> row((size_t)2 * wgs_reader_n_individuals(r) + 1);
    rc = reader_is_table(r) ? 0 : wgs_reader_next(r, row.data(), 1, &got);
    printf("    after the stop: rc %d, %lld rows\n", rc, (long long)got);
}

void trace_index(const std::string &f, const char *what, const std::string &idx)
{
    int64_t sites = -1;
    const int rc = wgs_reader_index_sites(f.c_str(), idx.c_str(), &sites);
    if (rc) printf("  %s: rc %d: %s\n", what, rc, g_err);
    else printf("  %s: %lld sites, index %s\n", what, (long long)sites, file_digest(idx, 24).c_str());
}

// the index pass in `nparts` parts; `damage`: raise the block count of part 0 before the merge
void trace_parts(const std::string &f, int nparts, bool damage)
{
    const std::string prefix = f + ".part", idx = f + ".pidx";
    printf("  in %d parts%s:", nparts, damage ? ", part 0 with a block count that its file does not hold" : "");
    bool ok = true;
    for (int k = 0; k < nparts; ++k) {
        const int rc = wgs_reader_index_part(f.c_str(), (prefix + "." + std::to_string(k)).c_str(), k, nparts, 3);
        printf(" %d", rc);
        if (rc) printf(" (%s)", g_err), ok = false;
    }
    printf("\n");
    if (damage && ok) {
        FILE *p = fopen((prefix + ".0").c_str(), "r+b");
        uint64_t nb = 0;
        if (p && fseek(p, 40, SEEK_SET) == 0 && fread(&nb, 8, 1, p) == 1) {
            nb += 100000;
            fseek(p, 40, SEEK_SET);
            fwrite(&nb, 8, 1, p);
        }
        if (p) fclose(p);
    }
    int64_t sites = -1;
    const int rc = ok ? wgs_reader_index_merge(f.c_str(), idx.c_str(), prefix.c_str(), nparts, 32768, 4096, &sites) : -1;
    if (rc > 0) printf("    merge: rc %d: %s\n", rc, g_err);
    else if (rc == 0) printf("    merge: %lld sites, index %s\n", (long long)sites, file_digest(idx, 24).c_str());
    for (int k = 0; k < nparts; ++k) {
        const std::string pp = prefix + "." + std::to_string(k);
        if (access(pp.c_str(), F_OK) == 0) printf("    %s was left behind\n", pp.c_str()), unlink(pp.c_str());
    }
    unlink(idx.c_str());
}

void trace_beagle(const std::string &f, bool damaged)
{
    printf("== %s\n", f.c_str());
    const std::string idx = f + ".idx", names = f + ".names";
    int64_t sites = -1, counted = -1, est = -1;
    int rc = wgs_reader_build_index(f.c_str(), idx.c_str(), names.c_str(), 32768, 4096, &sites);
    say_rc("wgs_reader_build_index", rc);
    if (rc == 0) {
        printf("  sites %lld, index %s, names %s\n", (long long)sites, file_digest(idx, 24).c_str(), file_digest(names, 0).c_str());
        trace_index(f, "wgs_reader_index_sites", idx);
        const std::string thin = f + ".idx3";
        rc = wgs_reader_build_index(f.c_str(), thin.c_str(), nullptr, 32768, 3, &counted);
        printf("  at most 3 access points: rc %d, %lld sites, index %s\n", rc, (long long)counted, file_digest(thin, 24).c_str());
        unlink(thin.c_str());
    }
    rc = wgs_reader_count_sites(f.c_str(), &counted);
    if (rc) say_rc("wgs_reader_count_sites", rc);
    else printf("  wgs_reader_count_sites: %lld\n", (long long)counted);
    rc = wgs_reader_estimate_sites(f.c_str(), &est);
    printf("  wgs_reader_estimate_sites: rc %d, %lld\n", rc, (long long)est);
    for (int nparts : {1, 2, 3}) trace_parts(f, nparts, false);

    const int64_t m = sites > 0 ? sites : 0;
    for (int threads : {1, 2, 7}) {
        printf(" threads %d\n", threads);
        wgs_reader *r = nullptr;
        rc = wgs_reader_open(f.c_str(), threads, &r);
        say_rc("wgs_reader_open", rc);
        if (rc) continue;
        if (threads == 1) {
            printf("  individuals %d, gl_cols %d, bgzf %d, table %d, samples", wgs_reader_n_individuals(r), reader_text_gl_cols(r), (int)reader_text_is_bgzf(r),
                   (int)reader_is_table(r));
            for (int i = 0; wgs_reader_sample_name(r, i); ++i) printf(" %s", wgs_reader_sample_name(r, i));
            printf("\n");
        }
        int64_t skipped = -1, nb = 0;
        rc = wgs_reader_skip_names(r, 10, &skipped);
        Fnv h;
        const char *sk = wgs_reader_chunk_sites(r, &nb);
        h.add(sk, (size_t)nb);
        printf("  skip_names: rc %d, %lld rows, names %016llx\n", rc, (long long)skipped, (unsigned long long)h.h);
        rc = wgs_reader_skip(r, 5, &skipped);
        printf("  skip: rc %d, %lld rows\n", rc, (long long)skipped);
        trace_rows("rows after the skips", r);
        wgs_reader_close(r);
        if (damaged) continue;
        const int64_t firsts[3] = {0, m / 3, m > 5 ? m - 5 : 0};
        for (int64_t first : firsts) {
            rc = wgs_reader_open_indexed(f.c_str(), idx.c_str(), first, threads, &r);
            if (rc) {
                say_rc("wgs_reader_open_indexed", rc);
                continue;
            }
            char what[64];
            snprintf(what, sizeof what, "indexed from row %lld", (long long)first);
            trace_rows(what, r);
            wgs_reader_close(r);
        }
    }
    for (int threads : {1, 7}) {
        for (int64_t limit : {(int64_t)-1, m / 2 + 3, (int64_t)0}) {
            wgs_reader *r = nullptr;
            if (wgs_reader_open(f.c_str(), threads, &r)) continue;
            printf(" text hand-over, threads %d, row limit %lld\n", threads, (long long)limit);
            trace_text(r, limit);
            wgs_reader_close(r);
        }
        if (!damaged) {
            wgs_reader *r = nullptr;
            if (wgs_reader_open_indexed(f.c_str(), idx.c_str(), m / 3, threads, &r) == 0) {
                printf(" text hand-over from row %lld of the index, threads %d\n", (long long)(m / 3), threads);
                trace_text(r, -1);
                wgs_reader_close(r);
            }
        }
        for (size_t max_members : {(size_t)0, (size_t)5}) {
            wgs_reader *r = nullptr;
            if (wgs_reader_open(f.c_str(), threads, &r)) continue;
            printf(" compressed hand-over, threads %d, max_members %zu\n", threads, max_members);
            trace_comp(r, max_members);
            wgs_reader_close(r);
        }
    }
    unlink(names.c_str());
}

void trace_table(const std::string &f)
{
    printf("== %s\n", f.c_str());
    for (int threads : {1, 7}) {
        wgs_reader *r = nullptr;
        int rc = wgs_reader_open_table(f.c_str(), threads, 2, &r);
        say_rc("wgs_reader_open_table", rc);
        if (rc) continue;
        printf(" threads %d: columns %d (%d), table %d, skipped %lld, bgzf %d\n", threads, wgs_reader_table_columns(r), reader_table_cols(r),
               (int)reader_is_table(r), (long long)reader_table_skip_lines(r), (int)reader_text_is_bgzf(r));
        trace_text(r, -1);
        wgs_reader_close(r);
        if (wgs_reader_open_table(f.c_str(), threads, 2, &r)) continue;
        std::vector<int32_t> rows((size_t)5000 * 6);
        std::vector<int64_t> linenos(5000);
        int64_t got = -1;
        rc = wgs_debug_reader_table_rows(r, 1, 6, rows.data(), 5000, &got, linenos.data());
        Fnv h;
        if (got > 0) h.add(rows.data(), (size_t)got * 6 * 4), h.add(linenos.data(), (size_t)got * 8);
        printf("  rows through the hand-over: rc %d, %lld rows %016llx\n", rc, (long long)got, (unsigned long long)h.h);
        wgs_reader_close(r);
        if (wgs_reader_open_table(f.c_str(), threads, 2, &r)) continue;
        printf(" compressed hand-over, threads %d\n", threads);
        trace_comp(r, 0);
        float x = 0;
        rc = wgs_reader_next(r, &x, 1, &got);
        say_rc("wgs_reader_next on a table", rc);
        rc = wgs_reader_skip(r, 1, &got);
        say_rc("wgs_reader_skip on a table", rc);
        wgs_reader_close(r);
    }
}

// a row with too few columns, through both ways to the rows
void trace_short(const std::string &f)
{
    printf("== %s\n", f.c_str());
    wgs_reader *r = nullptr;
    if (wgs_reader_open(f.c_str(), 2, &r)) return say_rc("wgs_reader_open", 2);
    trace_rows("rows", r);
    wgs_reader_close(r);
    if (wgs_reader_open(f.c_str(), 2, &r)) return;
    std::vector<float> rows((size_t)100 * 2 * wgs_reader_n_individuals(r));
    int64_t got = -1;
    const int rc = wgs_debug_reader_text_rows(r, 1, -1, rows.data(), 100, &got);
    printf("  rows through the hand-over: %lld\n", (long long)got);
    say_rc("wgs_debug_reader_text_rows", rc);
    wgs_reader_close(r);
}

void trace_refusals(const std::string &f)
{
    printf("== refusals (%s)\n", f.c_str());
    const std::string idx = f + ".idx";
    int64_t v = 0;
    wgs_reader *r = nullptr;
    float x = 0;
    say_rc("wgs_reader_open(null)", wgs_reader_open(nullptr, 1, &r));
    say_rc("wgs_reader_open(absent)", wgs_reader_open("absent.gz", 1, &r));
    say_rc("wgs_reader_open_table(null)", wgs_reader_open_table(nullptr, 1, 0, &r));
    say_rc("wgs_reader_open_table(skip < 0)", wgs_reader_open_table(f.c_str(), 1, -1, &r));
    say_rc("wgs_reader_open_table(absent)", wgs_reader_open_table("absent.txt", 1, 0, &r));
    say_rc("wgs_reader_build_index(null)", wgs_reader_build_index(nullptr, nullptr, nullptr, 0, 0, &v));
    say_rc("wgs_reader_build_index(absent)", wgs_reader_build_index("absent.gz", nullptr, nullptr, 0, 0, &v));
    say_rc("wgs_reader_index_part(null)", wgs_reader_index_part(f.c_str(), nullptr, 0, 1, 1));
    say_rc("wgs_reader_index_part(part out of range)", wgs_reader_index_part(f.c_str(), "p", 2, 2, 1));
    say_rc("wgs_reader_index_merge(null)", wgs_reader_index_merge(f.c_str(), nullptr, "p", 1, 0, 0, &v));
    say_rc("wgs_reader_index_merge(no parts)", wgs_reader_index_merge(f.c_str(), "i", "nothing", 2, 0, 0, &v));
    say_rc("wgs_reader_index_sites(null)", wgs_reader_index_sites(f.c_str(), nullptr, &v));
    say_rc("wgs_reader_index_sites(absent)", wgs_reader_index_sites(f.c_str(), "absent.idx", &v));
    say_rc("wgs_reader_open_indexed(null)", wgs_reader_open_indexed(f.c_str(), nullptr, 0, 1, &r));
    say_rc("wgs_reader_open_indexed(row < 0)", wgs_reader_open_indexed(f.c_str(), idx.c_str(), -1, 1, &r));
    say_rc("wgs_reader_open_indexed(row past the end)", wgs_reader_open_indexed(f.c_str(), idx.c_str(), 1 << 30, 1, &r));
    say_rc("wgs_reader_estimate_sites(null)", wgs_reader_estimate_sites(nullptr, &v));
    say_rc("wgs_reader_estimate_sites(absent)", wgs_reader_estimate_sites("absent.gz", &v));
    say_rc("wgs_reader_next(null)", wgs_reader_next(nullptr, &x, 1, &v));
    say_rc("wgs_reader_skip(null)", wgs_reader_skip(nullptr, 1, &v));
    say_rc("reader_text_next(null)", reader_text_next(nullptr, nullptr, nullptr));
    say_rc("reader_comp_next(null)", reader_comp_next(nullptr, nullptr, nullptr));
    say_rc("reader_text_start(null)", reader_text_start(nullptr, 1, 2, heap(), -1));
    say_rc("reader_comp_start(null)", reader_comp_start(nullptr, 1, 1, 2, heap()));
    printf("  null readers: %d %d %lld %d %d %lld\n", wgs_reader_n_individuals(nullptr), wgs_reader_table_columns(nullptr),
           (long long)reader_comp_bytes_left(nullptr), (int)reader_text_is_bgzf(nullptr), (int)reader_is_table(nullptr),
           (long long)wgs_debug_reader_text_chunks(nullptr));
    if (wgs_reader_open(f.c_str(), 1, &r) == 0) {
        say_rc("reader_text_start(no allocator)", reader_text_start(r, 1, 2, TextAllocator(), -1));
        say_rc("reader_text_start(no buffers)", reader_text_start(r, 1, 0, heap(), -1));
        say_rc("reader_text_next(not started)", reader_text_next(r, nullptr, nullptr));
        say_rc("reader_text_start", reader_text_start(r, 1, 2, heap(), -1));
        say_rc("reader_text_start(twice)", reader_text_start(r, 1, 2, heap(), -1));
        say_rc("reader_comp_start(text hand-over running)", reader_comp_start(r, 1, 1, 2, heap()));
        wgs_reader_close(r);
    }
    // the file changes after its index was written
    struct timespec ts[2] = {{1000000000, 0}, {1000000000, 5}};
    utimensat(AT_FDCWD, f.c_str(), ts, 0);
    say_rc("wgs_reader_index_sites(stale)", wgs_reader_index_sites(f.c_str(), idx.c_str(), &v));
    say_rc("wgs_reader_open_indexed(stale)", wgs_reader_open_indexed(f.c_str(), idx.c_str(), 0, 1, &r));
}

bool starts(const std::string &s, const char *p) { return s.compare(0, strlen(p), p) == 0; }

}  // namespace

int main(int argc, char **argv)
{
    std::string first_bgzf;
    for (int i = 1; i < argc; ++i) {
        const std::string f = argv[i];
        if (starts(f, "table")) trace_table(f);
        else if (starts(f, "bad_short")) trace_short(f);
        else trace_beagle(f, starts(f, "bad_"));
        if (first_bgzf.empty() && starts(f, "beagle_b")) first_bgzf = f;
    }
    if (!first_bgzf.empty()) {
        printf("== %s, damaged part file\n", first_bgzf.c_str());
        trace_parts(first_bgzf, 2, true);
        trace_refusals(first_bgzf);
    }
    return 0;
}
