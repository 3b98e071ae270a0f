// Streamed Beagle reader -- the native counterpart of reader_cy.readBeagle (reader_cy.pyx:16-77).
//
// The reference pipes `gunzip -c` through Python, tokenises every line with strtok(" \t\n") and
// converts with atof into a vector<vector<float>> that is then copied into a NumPy array (two
// copies of the matrix in RAM, ~30 k sites/s).  Here: zlib inflate into a large buffer, lines
// parsed in parallel by worker threads straight into the caller's float32 (rows, 2n) chunk --
// chunk by chunk, so a file larger than host RAM can be streamed into device slabs.
//
// Parity rules kept (reader_cy.pyx:35-66): header tokens after the first three name the GL
// columns, every third one (c % 3 == 1) is a sample name; per line token 0 is the site name, two
// allele tokens are skipped, of every GL triple the first two values are kept and the third
// dropped; a value is atof(token) rounded to float32.  atof == strtod: decimal tokens with at
// most 15 significant digits and no exponent take the exact fast path (integer mantissa / power
// of ten, one correctly rounded division -- identical to strtod for such inputs); anything else
// (exponents, inf/nan, hex) goes through strtod itself.
//
// The reader is split into units; comments elsewhere cite functions as "reader.cpp: NAME".  Where those live now:
//   is_delim                      reader_impl.h
//   parse_f6, parse_double        here
//   BlockInflater                 bgzf.h (with the BGZF member walk, pread_slices and RawBuf)
//   GzSource                      gz_source.h
//   list_lines, text_producer,
//   comp_producer                 reader_pipes.cpp (the two hand-overs of reader_text.h, on one chunk queue)
//   the index pass and its files  reader_index.cpp
// Here: the token parsers, fill, open / open_table / open_indexed, next / skip, and the debug hooks.
#include <stdio.h>

#include <algorithm>

#include "reader_impl.h"

namespace {

const double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                           1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// atof of the token [p, e) (no delimiters inside).  Decimal tokens -- [sign] digits [. digits] [e [sign] digits] -- whose
// mantissa fits 53 bits and whose net power of ten is at most 22 in magnitude take the exact path: one correctly
// rounded multiplication or division of two exactly representable numbers, which is the correctly rounded value of
// the token, i.e. strtod's result.  Everything else (longer mantissas, inf/nan, hex, trailing junk) is strtod's.
// ingest.hip holds the device twin of this function (tokenise_kernel): the two must accept the same tokens.
inline double parse_double(const char *p, const char *e)
{
    const char *q = p;
    bool neg = false;
    if (q < e && (*q == '-' || *q == '+')) neg = *q++ == '-';
    uint64_t mant = 0;
    int digits = 0, frac = 0, seen = 0;
    bool dot = false, ok = true;
    for (; q < e; ++q) {
        const char c = *q;
        if (c >= '0' && c <= '9') {
            ++seen;
            if (mant == 0 && c == '0') {                     // zeros before the first significant digit
                if (dot) ++frac;
                continue;
            }
            if (++digits > 15) break;
            mant = mant * 10 + (uint64_t)(c - '0');
            if (dot) ++frac;
        } else if (c == '.' && !dot) {
            dot = true;
        } else {
            break;
        }
    }
    int ex = 0;
    if (q < e && (*q == 'e' || *q == 'E') && seen > 0 && digits <= 15) {
        const char *x = q + 1;
        bool xneg = false;
        if (x < e && (*x == '-' || *x == '+')) xneg = *x++ == '-';
        int xd = 0;
        for (; x < e && *x >= '0' && *x <= '9' && xd < 4; ++x, ++xd) ex = ex * 10 + (*x - '0');
        if (xd == 0 || xd > 3) ok = false;                   // "1e", "1e+": atof stops before the 'e'
        if (xneg) ex = -ex;
        q = x;
    }
    const int net = ex - frac;
    if (ok && q == e && seen > 0 && digits <= 15 && net >= -22 && net <= 22) {
        const double v = net < 0 ? (double)mant / kPow10[-net] : (double)mant * kPow10[net];
        return neg ? -v : v;
    }
    char tmp[64];
    const size_t len = (size_t)(e - p);
    if (len < sizeof tmp) {
        memcpy(tmp, p, len);
        tmp[len] = 0;
        return strtod(tmp, nullptr);
    }
    std::string str(p, e);
    return strtod(str.c_str(), nullptr);
}

// The token almost every Beagle file consists of: "d.dddddd" (ANGSD prints %f) followed by a delimiter or the end of
// the line.  Eight bytes are checked and converted at once: XOR with "0.000000" leaves the digit values (and 0 for the
// point), the pairwise multiply-adds of the usual eight-digit trick give d0 d2 .. d7 0 = 10 * mantissa, and the value is
// that integer / 1e7 -- one correctly rounded division of two exactly representable numbers, i.e. strtod's result.
inline bool parse_f6(const char *p, const char *e, double *v)
{
    if (e - p < 8 || (e - p > 8 && !is_delim(p[8]))) return false;
    uint64_t w;
    memcpy(&w, p, 8);
    uint64_t d = w ^ 0x3030303030302E30ull;
    if ((((d + 0x7676767676767676ull) | d) & 0x8080808080808080ull) || (d & 0xFF00ull)) return false;
    d = (d >> 8) | (d & 0xFF);                               // first digit, then the six decimals, then 0
    d = d * 10 + (d >> 8);
    const uint64_t mask = 0x000000FF000000FFull;
    d = (((d & mask) * (100 + (1000000ull << 32))) + (((d >> 16) & mask) * (1 + (10000ull << 32)))) >> 32;
    *v = (double)(uint32_t)d / 1e7;
    return true;
}

struct Line {
    const char *begin, *end;   // without the newline
};

bool fill(wgs_reader *r)
{
    // keep the unconsumed tail, append more inflated bytes
    if (r->pos > 0) {
        memmove(r->buf.data(), r->buf.data() + r->pos, r->len - r->pos);
        r->len -= r->pos;
        r->pos = 0;
    }
    // a single line longer than the buffer; a whole 64 KiB BGZF block, or one batch of stretches between access
    // points, must fit behind the tail
    const size_t want = r->src.want_room();
    if (r->buf.size() - r->len < want && !r->buf.resize(r->src.segmented ? r->len + want : r->buf.size() * 2)) return false;
    const size_t room = r->buf.size() - r->len;
    const size_t limit = r->len + std::min(room, std::max(r->fill_cap, want));
    while (!r->eof && r->len < limit) {
        const bool batch = r->src.segmented;
        const long got = r->src.read(r->buf.data() + r->len, limit - r->len);
        if (got == -2) break;                                 // the next block does not fit any more; enough for now
        if (got < 0) return false;
        if (got == 0) {
            r->eof = true;
            break;
        }
        r->len += (size_t)got;
        if (batch) break;                                     // one parallel batch per call (a second would be a partial one)
    }
    return true;
}

// Parse one data line into out[0 .. 2*n_inds); returns false when the line is short.
bool parse_line(const wgs_reader *r, const Line &ln, float *out, std::string *site)
{
    const char *p = ln.begin, *e = ln.end;
    auto next = [&](const char *&tb, const char *&te) {
        while (p < e && is_delim(*p)) ++p;
        if (p >= e) return false;
        tb = p;
        while (p < e && !is_delim(*p)) ++p;
        te = p;
        return true;
    };
    const char *tb, *te;
    if (!next(tb, te)) return false;
    site->assign(tb, te);                                  // reader_cy.pyx:56-57
    if (!next(tb, te) || !next(tb, te)) return false;      // allele1, allele2 (reader_cy.pyx:59-60)
    // a header whose GL column count is not a multiple of 3 leaves a partial individual: the reference
    // parses those columns but only keeps the first 2 * (n // 3) values of each row (reader_cy.pyx:48-49,
    // 71-75), so they are not read at all here -- every row is exactly 2 * n_inds floats
    for (int i = 0; i < r->n_inds; ++i) {
        // fast path: "\td.dddddd\td.dddddd\t<anything>" -- one delimiter, two fixed-format values, the third skipped
        if (e - p >= 19 && is_delim(p[0])) {
            double a, b;
            if (parse_f6(p + 1, e, &a) && parse_f6(p + 10, e, &b)) {
                const char *q = p + 19;
                while (q < e && !is_delim(*q)) ++q;
                if (q > p + 19) {                                         // the third value is there
                    *out++ = (float)a;
                    *out++ = (float)b;
                    p = q;
                    continue;
                }
            }
        }
        for (int j = 0; j < 3; ++j) {
            if (!next(tb, te)) return false;
            if (j < 2) *out++ = (float)parse_double(tb, te);              // reader_cy.pyx:62-66
        }
    }
    return true;
}

}  // namespace

// Header line (reader_cy.pyx:35-49): tokens after the first three are GL columns, every third names a sample.
void parse_header(const char *p, const char *hend, std::vector<std::string> &samples, int &gl_cols)
{
    int tok = 0;
    samples.clear();
    while (p < hend) {
        while (p < hend && is_delim(*p)) ++p;
        if (p >= hend) break;
        const char *tb = p;
        while (p < hend && !is_delim(*p)) ++p;
        ++tok;
        if (tok > 3 && (tok - 3) % 3 == 1) samples.emplace_back(tb, p);
    }
    gl_cols = tok > 3 ? tok - 3 : 0;
}

extern "C" {

int wgs_reader_open(const char *path, int threads, wgs_reader **out)
{
    if (!path || !out) {
        wgs_set_error("null argument");
        return 2;
    }
    wgs_reader *r = new wgs_reader();
    if (!r->src.open(path, nullptr)) {
        wgs_set_error("cannot open Beagle file %s", path);
        delete r;
        return 2;
    }
    r->threads = threads > 0 ? threads : 1;
    r->src.try_bgzf(r->threads);
    if (!r->buf.resize(64u << 20)) {
        wgs_set_error("out of memory");
        delete r;
        return 1;
    }
    if (r->src.bgzf) r->fill_cap = 1u << 20;
    if (!fill(r)) {
        wgs_set_error("read error in %s", path);
        delete r;
        return 1;
    }
    const char *nl = (const char *)memchr(r->buf.data(), '\n', r->len);
    while (!nl && !r->eof) {
        if (!fill(r)) break;
        nl = (const char *)memchr(r->buf.data(), '\n', r->len);
    }
    const char *hend = nl ? nl : r->buf.data() + r->len;
    parse_header(r->buf.data(), hend, r->samples, r->gl_cols);
    r->n_inds = r->gl_cols / 3;
    r->pos = nl ? (size_t)(nl - r->buf.data()) + 1 : r->len;
    r->fill_cap = (size_t)-1;
    *out = r;
    return 0;
}

/* An integer table (allele depths, ANGSD counts): plain text, gzip or BGZF, told apart by the file's first bytes.  The first
 * skip_lines lines are dropped whatever they hold; the first data line behind them -- not blank, not a whole-line '#' comment, as
 * np.loadtxt sees it -- gives the column count and stays unread. */
int wgs_reader_open_table(const char *path, int threads, int skip_lines, wgs_reader **out)
{
    if (!path || !out || skip_lines < 0) {
        wgs_set_error("bad argument");
        return 2;
    }
    wgs_reader *r = new wgs_reader();
    if (!r->src.open(path, nullptr)) {
        wgs_set_error("cannot open %s", path);
        delete r;
        return 2;
    }
    r->table = true;
    r->skip_lines = skip_lines;
    r->threads = threads > 0 ? threads : 1;
    unsigned char magic[2] = {0, 0};
    const size_t got = fread(magic, 1, 2, r->src.fp);
    fseeko(r->src.fp, 0, SEEK_SET);
    if (got < 2 || magic[0] != 0x1f || magic[1] != 0x8b) {
        r->src.plain = true;
        std::vector<unsigned char>().swap(r->src.in);      // the gzip stream's staging buffer is not needed
    } else {
        r->src.try_bgzf(r->threads, 4u << 20);
    }
    if (!r->buf.resize(1u << 20)) {
        wgs_set_error("out of memory");
        delete r;
        return 1;
    }
    r->fill_cap = 1u << 20;
    // the header lines are consumed; what follows stays in the buffer (blank and comment lines before the first row too: the
    // hand-over's line numbering counts them).  Offsets are relative to r->pos: fill() moves the unread text to the front.
    int64_t skipped = 0;
    for (size_t at = 0;;) {
        const char *p = r->buf.data() + r->pos + at, *e = r->buf.data() + r->len;
        const char *nl = p < e ? (const char *)memchr(p, '\n', (size_t)(e - p)) : nullptr;
        if (!nl && !r->eof) {
            if (!fill(r)) {
                wgs_set_error("read error in %s", path);
                delete r;
                return 1;
            }
            continue;
        }
        if (p >= e) break;                                   // the file ends before a data line
        const char *le = nl ? nl : e;
        const size_t next = (size_t)(le - (r->buf.data() + r->pos)) + (nl ? 1 : 0);
        if (skipped < skip_lines) {
            ++skipped;
            r->pos += next;
            continue;
        }
        const char *q = p;
        while (q < le && is_delim(*q)) ++q;
        if (q < le && *q != '#') {
            int cols = 0;
            while (q < le && *q != '#') {
                while (q < le && !is_delim(*q) && *q != '#') ++q;
                ++cols;
                while (q < le && is_delim(*q)) ++q;
            }
            r->table_cols = cols;
            break;
        }
        if (!nl) break;
        at = next;
    }
    r->fill_cap = (size_t)-1;
    r->host_peak = std::max(r->buf.size(), r->src.bgzf ? r->src.cbuf.size() : r->src.in.size());
    *out = r;
    return 0;
}

int wgs_reader_table_columns(wgs_reader *r) { return r && r->table ? r->table_cols : 0; }

void wgs_reader_close(wgs_reader *r)
{
    if (!r) return;
    reader_comp_stop(r);
    reader_text_stop(r);
    delete r;
}

/* A reader positioned so that the next row it returns is `first_row` (0-based site index): it starts inflating
 * at the last access point at or before that row and skips the few lines in between without parsing. */
int wgs_reader_open_indexed(const char *path, const char *index_path, int64_t first_row, int threads, wgs_reader **out)
{
    if (!path || !index_path || !out || first_row < 0) {
        wgs_set_error("bad argument");
        return 2;
    }
    BeagleIndex idx;
    if (!index_matches_file(index_path, path, idx)) {
        wgs_set_error("%s is not an index of %s", index_path, path);
        return 2;
    }
    // data row r is non-blank line r + 1; an access point serves it when lines_before <= r + 1 (it may sit inside
    // line lines_before, whose remainder is then skipped: that costs one more line of margin)
    const AccessPoint *best = nullptr;
    for (const auto &a : idx.points) {
        const int64_t first_full = a.lines_before + (a.at_line_start ? 0 : 1);
        if (first_full <= first_row + 1 && (!best || a.out > best->out)) best = &a;
    }
    wgs_reader *r = new wgs_reader();
    r->samples = idx.samples;
    r->gl_cols = idx.gl_cols;
    r->n_inds = idx.gl_cols / 3;
    r->threads = threads > 0 ? threads : 1;
    if (!r->buf.resize(64u << 20)) {
        wgs_set_error("out of memory");
        delete r;
        return 1;
    }
    if (!r->src.open(path, best)) {
        wgs_set_error("cannot open Beagle file %s at its access point", path);
        delete r;
        return 2;
    }
    if (!best || best->member_start) r->src.try_bgzf(r->threads);
    if (r->src.bgzf) r->fill_cap = 1u << 20;
    const bool have_best = best != nullptr;
    const int64_t best_lines = best ? best->lines_before : 0;
    const bool best_line_start = best ? best->at_line_start != 0 : true, best_content = best ? best->content != 0 : false;
    if (!r->src.bgzf && r->threads > 1) {                    // plain gzip: inflate the stretches between access points in parallel
        std::vector<AccessPoint> segs;
        if (best) {
            segs.push_back(*best);
        } else {
            AccessPoint start;
            start.member_start = 1;
            start.at_line_start = 1;
            segs.push_back(start);
        }
        for (auto &a : idx.points)
            if (a.out > segs.back().out) segs.push_back(std::move(a));   // idx.points (and `best`) are spent from here on
        best = nullptr;
        r->src.use_segments(path, std::move(segs), r->threads);
    }
    int64_t line = 0;            // non-blank line index of the next complete line in the buffer
    if (have_best) {
        if (!fill(r)) {
            wgs_set_error("read error in %s", path);
            delete r;
            return 1;
        }
        line = best_lines;
        if (!best_line_start) {                          // drop the tail of the line the access point sits in
            bool content = best_content;
            for (;;) {
                const char *b = r->buf.data() + r->pos;
                const char *nl = (const char *)memchr(b, '\n', r->len - r->pos);
                const char *e = nl ? nl : r->buf.data() + r->len;
                for (const char *t = b; t < e && !content; ++t) content = !is_delim(*t);
                r->pos = (size_t)(e - r->buf.data()) + (nl ? 1 : 0);
                if (nl || r->eof) break;
                if (!fill(r)) {
                    wgs_set_error("read error in %s", path);
                    delete r;
                    return 1;
                }
                if (r->eof && r->pos >= r->len) break;
            }
            line += content ? 1 : 0;
        }
    } else {
        line = 0;                                        // from the first byte: the header is line 0
    }
    // skip whole lines up to the wanted row (line index first_row + 1); from the start that includes the header
    int64_t to_skip = first_row + 1 - line, got = 0;
    if (to_skip < 0) {
        wgs_set_error("index of %s is inconsistent", path);
        delete r;
        return 1;
    }
    if (to_skip > 0 && (wgs_reader_skip(r, to_skip, &got) != 0 || got != to_skip)) {
        if (got != to_skip) wgs_set_error("Beagle file %s is shorter than its index says", path);
        delete r;
        return 1;
    }
    r->lines_read = first_row;
    r->fill_cap = (size_t)-1;
    *out = r;
    return 0;
}

int wgs_reader_n_individuals(wgs_reader *r) { return r ? r->n_inds : 0; }

const char *wgs_reader_sample_name(wgs_reader *r, int i)
{
    if (!r || i < 0 || i >= (int)r->samples.size()) return nullptr;
    return r->samples[i].c_str();
}

int wgs_reader_next(wgs_reader *r, float *rows, int64_t max_rows, int64_t *nrows)
{
    if (!r || !rows || !nrows || max_rows < 0) {
        wgs_set_error("bad argument");
        return 2;
    }
    if (r->table) {
        wgs_set_error("the reader was opened for an integer table, not a Beagle file");
        return 2;
    }
    r->chunk_sites.clear();
    int64_t done = 0;
    const size_t row_floats = (size_t)2 * r->n_inds;
    std::vector<Line> lines;
    std::vector<std::string> sites;
    while (done < max_rows) {
        // complete lines available in the buffer
        lines.clear();
        size_t scan = r->pos;
        while ((int64_t)lines.size() < max_rows - done && scan < r->len) {
            const char *nl = (const char *)memchr(r->buf.data() + scan, '\n', r->len - scan);
            if (!nl) {
                if (!r->eof) break;
                nl = r->buf.data() + r->len;                 // last line without newline
            }
            const char *b = r->buf.data() + scan, *e = nl;
            scan = (size_t)(nl - r->buf.data()) + (nl < r->buf.data() + r->len ? 1 : 0);
            const char *t = b;
            while (t < e && is_delim(*t)) ++t;
            if (t < e) lines.push_back({b, e});              // blank lines are skipped
            if (nl == r->buf.data() + r->len) break;
        }
        if (lines.empty()) {
            r->pos = scan;
            if (r->eof && r->pos >= r->len) break;
            const size_t before = r->len - r->pos;
            if (!fill(r)) {
                wgs_set_error("read error while inflating the Beagle file");
                return 1;
            }
            if (r->eof && r->len - r->pos == before && before == 0) break;
            continue;
        }
        sites.assign(lines.size(), std::string());
        const int T = (int)std::min<size_t>((size_t)r->threads, lines.size());
        std::vector<int64_t> bad(T, -1);
        run_threads(T, [&](int t) {
            for (size_t i = (size_t)t; i < lines.size(); i += (size_t)T)
                if (!parse_line(r, lines[i], rows + ((size_t)done + i) * row_floats, &sites[i]) && bad[t] < 0) bad[t] = (int64_t)i;
        });
        for (int t = 0; t < T; ++t)
            if (bad[t] >= 0) {
                wgs_set_error("Beagle data line %lld has fewer than %d genotype-likelihood columns",
                              (long long)(r->lines_read + done + bad[t] + 2), r->gl_cols);
                return 2;
            }
        for (auto &s : sites) {
            r->chunk_sites += s;
            r->chunk_sites += '\n';
        }
        done += (int64_t)lines.size();
        r->pos = scan;
    }
    r->lines_read += done;
    *nrows = done;
    return 0;
}

static int skip_impl(wgs_reader *r, int64_t max_rows, int64_t *nrows, bool names);

/* Skip up to max_rows data lines without parsing them (a rank that owns a later SNP range). */
int wgs_reader_skip(wgs_reader *r, int64_t max_rows, int64_t *nrows) { return skip_impl(r, max_rows, nrows, false); }

/* Same, but keep the site names of the skipped lines (wgs_reader_chunk_sites): a names-only pass. */
int wgs_reader_skip_names(wgs_reader *r, int64_t max_rows, int64_t *nrows) { return skip_impl(r, max_rows, nrows, true); }

static int skip_impl(wgs_reader *r, int64_t max_rows, int64_t *nrows, bool names)
{
    if (!r || !nrows || max_rows < 0) {
        wgs_set_error("bad argument");
        return 2;
    }
    if (r->table) {
        wgs_set_error("the reader was opened for an integer table, not a Beagle file");
        return 2;
    }
    if (names) r->chunk_sites.clear();
    int64_t done = 0;
    while (done < max_rows) {
        bool progressed = false;
        while (done < max_rows && r->pos < r->len) {
            const char *b = r->buf.data() + r->pos;
            const char *nl = (const char *)memchr(b, '\n', r->len - r->pos);
            if (!nl) {
                if (!r->eof) break;
                nl = r->buf.data() + r->len;
            }
            const char *t = b;
            while (t < nl && is_delim(*t)) ++t;
            done += t < nl;                                   // blank lines do not count
            if (names && t < nl) {
                const char *e = t;
                while (e < nl && !is_delim(*e)) ++e;
                r->chunk_sites.append(t, e);
                r->chunk_sites += '\n';
            }
            r->pos = (size_t)(nl - r->buf.data()) + (nl < r->buf.data() + r->len ? 1 : 0);
            progressed = true;
        }
        if (done >= max_rows) break;
        if (r->eof && r->pos >= r->len) break;
        const size_t before = r->len - r->pos;
        if (!fill(r)) {
            wgs_set_error("read error while inflating the Beagle file");
            return 1;
        }
        if (!progressed && r->eof && r->len - r->pos == before && before == 0) break;
    }
    r->lines_read += done;
    *nrows = done;
    return 0;
}

const char *wgs_reader_chunk_sites(wgs_reader *r, int64_t *bytes)
{
    if (!r) return nullptr;
    if (bytes) *bytes = (int64_t)r->chunk_sites.size();
    return r->chunk_sites.c_str();
}

}  // extern "C"

void reader_add_lines_read(wgs_reader *r, int64_t rows) { r->lines_read += rows; }

int reader_text_parse_line(const wgs_reader *r, const char *b, const char *e, float *out)
{
    std::string site;
    return parse_line(r, Line{b, e}, out, &site) ? 0 : 1;
}

int reader_text_n_inds(const wgs_reader *r) { return r->n_inds; }
int reader_text_gl_cols(const wgs_reader *r) { return r->gl_cols; }
int64_t reader_text_lines_read(const wgs_reader *r) { return r->lines_read; }

bool reader_is_table(const wgs_reader *r) { return r && r->table; }
int reader_table_cols(const wgs_reader *r) { return r->table_cols; }
int64_t reader_table_skip_lines(const wgs_reader *r) { return r->skip_lines; }

int reader_table_parse_line(const char *b, const char *e, int need, int32_t *out, int *bad_col)
{
    const char *hash = (const char *)memchr(b, '#', (size_t)(e - b));
    if (hash) e = hash;
    const char *p = b;
    for (int col = 0; col < need; ++col) {
        while (p < e && is_delim(*p)) ++p;
        if (p >= e) return 1;
        const char *q = p;
        bool neg = false;
        if (*q == '+' || *q == '-') neg = *q++ == '-';
        int64_t v = 0;
        int digits = 0;
        for (; q < e && *q >= '0' && *q <= '9'; ++q, ++digits)
            if (v < ((int64_t)1 << 40)) v = v * 10 + (*q - '0');
        if (neg) v = -v;
        if (digits == 0 || (q < e && !is_delim(*q))) {
            // np.loadtxt still reads an integer column "via a float" (deprecated since NumPy 1.23): a plain decimal or exponent
            // form, truncated towards zero.  Nothing with letters other than the exponent's (inf, nan, hex).
            const char *te = p;
            bool plain = true;
            while (te < e && !is_delim(*te)) {
                const char c = *te++;
                if (!((c >= '0' && c <= '9') || c == '.' || c == 'e' || c == 'E' || c == '+' || c == '-')) plain = false;
            }
            const std::string tok(p, te);
            char *stop = nullptr;
            const double f = plain ? strtod(tok.c_str(), &stop) : 0.0;
            if (!plain || stop != tok.c_str() + tok.size() || !(f > -2147483649.0 && f < 2147483648.0)) {
                if (bad_col) *bad_col = col + 1;
                return 3;
            }
            v = (int64_t)f;
            q = te;
        }
        if (v > INT32_MAX || v < INT32_MIN) {
            if (bad_col) *bad_col = col + 1;
            return 3;
        }
        out[col] = (int32_t)v;
        p = q;
    }
    return 0;
}

// ordinary memory where the device ingest takes page-locked memory
static TextAllocator malloc_allocator()
{
    TextAllocator a;
    a.alloc = [](size_t n, void *) { return malloc(n); };
    a.release = [](void *p, void *) { free(p); };
    return a;
}

extern "C" {

/* Test hook (needs no GPU): the rows of wgs_reader_next, but through the text hand-over -- the producer thread, the
 * carried partial lines, the parallel newline scan, the row limit -- with ordinary memory for the buffers and the host
 * parser in place of the device tokeniser.  One call drains the reader: rows[max_rows][2n], site names through
 * wgs_reader_chunk_sites. */
int64_t wgs_debug_reader_text_chunks(wgs_reader *r) { return r ? r->text_chunks : 0; }

int wgs_debug_reader_text_rows(wgs_reader *r, int64_t chunk_bytes, int64_t limit_rows, float *rows, int64_t max_rows, int64_t *nrows)
{
    if (!r || !nrows) {                                    // rows == NULL: only drain the hand-over (inflate + line lists), for timing
        wgs_set_error("bad argument");
        return 2;
    }
    if (int rc = reader_text_start(r, (size_t)chunk_bytes, 2, malloc_allocator(), limit_rows)) return rc;
    r->chunk_sites.clear();
    const size_t row_floats = (size_t)2 * r->n_inds;
    int64_t done = 0;
    int rc = 0;
    for (;;) {
        TextChunk *c = nullptr;
        if ((rc = reader_text_next(r, &c, nullptr)) != 0 || !c) break;
        if (c->first_row != done) rc = 1, wgs_set_error("text chunks out of order");
        if (!rows) done += (int64_t)c->begin.size();
        for (size_t i = 0; rows && i < c->begin.size() && !rc; ++i) {
            if (done >= max_rows) {
                rc = 2;
                wgs_set_error("more rows than the caller has room for");
            } else if (reader_text_parse_line(r, c->data + c->begin[i], c->data + c->end[i], rows + (size_t)done * row_floats)) {
                rc = 2;
                wgs_set_error("Beagle data line %lld has fewer than %d genotype-likelihood columns", (long long)(r->lines_read + done + 2), r->gl_cols);
            } else {
                ++done;
            }
        }
        r->chunk_sites += c->names;
        reader_text_release(r, c);
        if (rc) break;
    }
    reader_text_stop(r);
    *nrows = done;
    return rc;
}

/* Test hook (needs no GPU): an integer table through the text hand-over, every listed line parsed by reader_table_parse_line:
 * rows[max_rows][need], linenos[max_rows] = each row's 1-based line number in the file.  rc 2 with the message the device ingest
 * gives when a line has too few columns or a token np.loadtxt refuses. */
int wgs_debug_reader_table_rows(wgs_reader *r, int64_t chunk_bytes, int32_t need, int32_t *rows, int64_t max_rows, int64_t *nrows, int64_t *linenos)
{
    if (!r || !r->table || !rows || !nrows || need < 1) {
        wgs_set_error("bad argument");
        return 2;
    }
    if (int rc = reader_text_start(r, (size_t)chunk_bytes, 2, malloc_allocator(), -1)) return rc;
    int64_t done = 0;
    int rc = 0;
    for (;;) {
        TextChunk *c = nullptr;
        if ((rc = reader_text_next(r, &c, nullptr)) != 0 || !c) break;
        for (size_t i = 0; i < c->begin.size() && !rc; ++i) {
            const long long line = (long long)(r->skip_lines + c->first_line + c->lineno[i] + 1);
            int bad_col = 0;
            if (done >= max_rows) {
                rc = 2;
                wgs_set_error("more rows than the caller has room for");
                break;
            }
            const int k = reader_table_parse_line(c->data + c->begin[i], c->data + c->end[i], need, rows + (size_t)done * need, &bad_col);
            if (k == 1) rc = 2, wgs_set_error("line %lld has fewer than %d columns", line, need);
            else if (k) rc = 2, wgs_set_error("line %lld, column %d: not an integer np.loadtxt reads as int32", line, bad_col);
            else {
                if (linenos) linenos[done] = line;
                ++done;
            }
        }
        reader_text_release(r, c);
        if (rc) break;
    }
    reader_text_stop(r);
    *nrows = done;
    return rc;
}

int wgs_debug_table_parse_line(const char *line, int64_t len, int32_t need, int32_t *out)
{
    int bad_col = 0;
    return reader_table_parse_line(line, line + len, need, out, &bad_col);
}

/* Debug / tests: the COMPRESSED hand-over (reader_text.h: CompChunk -- what the device-resident ingest consumes) driven on the
 * host: every chunk's pre-inflated text and members (inflated here with the host's inflater) appended to text[0 .. cap);
 * info[0] = chunks, info[1] = members, info[2] = largest text of one chunk, info[3] = chunks of pre-inflated text. */
int wgs_debug_reader_comp_text(wgs_reader *r, int64_t comp_bytes, int64_t text_cap, int nbuf, char *text, int64_t cap, int64_t *bytes, int64_t *info)
{
    if (!r || !text || !bytes || !info) {
        wgs_set_error("bad argument");
        return 2;
    }
    if (int rc = reader_comp_start(r, (size_t)comp_bytes, (size_t)text_cap, nbuf, malloc_allocator())) return rc;
    int64_t at = 0;
    int rc = 0;
    info[0] = info[1] = info[2] = info[3] = 0;
    for (;;) {
        CompChunk *c = nullptr;
        if ((rc = reader_comp_next(r, &c, nullptr)) != 0 || !c) break;
        const int64_t here = (int64_t)c->pre_len + (int64_t)c->text_bytes;
        if (at + here > cap) {
            rc = 2;
            wgs_set_error("more text than the caller has room for");
        } else {
            if (c->pre_len) memcpy(text + at, c->pre_text, c->pre_len);
            at += (int64_t)c->pre_len;
            for (size_t i = 0; i < c->isize.size() && !rc; ++i) {
                if (!reader_inflate_member(c->comp + c->in_off[i], c->in_len[i], c->isize[i], reinterpret_cast<unsigned char *>(text + at))) {
                    rc = 1;
                    wgs_set_error("read error in the BGZF file (corrupt block)");
                }
                at += c->isize[i];
            }
        }
        info[0] += 1;
        info[1] += (int64_t)c->isize.size();
        info[2] = std::max<int64_t>(info[2], here);
        info[3] += c->pre_len ? 1 : 0;
        const bool last = c->last;
        reader_comp_release(r, c);
        if (rc || last) break;
    }
    reader_comp_stop(r);
    *bytes = at;
    return rc;
}

}  // extern "C"
