// The two hand-overs of the streamed reader to the device ingest (reader_text.h): inflated text in whole lines, and -- for
// BGZF files -- compressed members.  Each is a producer thread beside the consumer, on one chunk queue.  Host code only.
#include <stdio.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>

#include "reader_impl.h"

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- the chunk queue ---------------------------------------------------------------------------------------------
// The producer thread takes chunks off the free list, fills them and publishes them in file order; the consumer takes
// them with next() and gives them back with release().  The last chunk, or a failure, finishes the queue: next() then
// returns what is still ready, and after that no chunk and the failure's code.
template <typename Chunk>
struct ChunkQueue {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Chunk *> free_q, ready_q;
    bool finished = false, stop = false;
    int rc = 0;
    std::string err;

    // ---- the producer's side
    bool take_free(Chunk *&c)                // false: the consumer has stopped the hand-over
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || !free_q.empty(); });
        if (stop) return false;
        c = free_q.front();
        free_q.pop_front();
        return true;
    }
    void publish(Chunk *c, bool last) { put(ready_q, c, last); }
    void recycle(Chunk *c, bool last) { put(free_q, c, last); }
    void fail(int code, const char *msg)
    {
        std::lock_guard<std::mutex> lk(mu);
        rc = code;
        err = msg;
        finished = true;
        cv.notify_all();
    }
    // ---- the consumer's side
    int next(Chunk **out, double *waited_s)
    {
        const double t0 = now_s();
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !ready_q.empty() || finished; });
        if (waited_s) *waited_s = now_s() - t0;
        *out = nullptr;
        if (!ready_q.empty()) {
            *out = ready_q.front();
            ready_q.pop_front();
            return 0;
        }
        if (rc) wgs_set_error("%s", err.c_str());
        return rc;
    }
    void release(Chunk *c) { put(free_q, c, false); }
    void stop_and_join()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
            cv.notify_all();
        }
        if (th.joinable()) th.join();
    }

private:
    void put(std::deque<Chunk *> &q, Chunk *c, bool last)
    {
        std::lock_guard<std::mutex> lk(mu);
        q.push_back(c);
        if (last) finished = true;
        cv.notify_all();
    }
};

// ---- text hand-over to the device tokeniser ----------------------------------------------------------------------
// A producer thread inflates ahead into caller-allocated (pinned) buffers, cuts each at its last newline, carries
// the partial line into the next buffer, and lists the non-blank lines -- newline scan and first tokens (site names)
// on all of the reader's threads.  Everything per VALUE happens on the GPU.
struct TextPipe : ChunkQueue<TextChunk> {
    std::vector<TextChunk *> all;
    TextAllocator alloc;
    size_t chunk_bytes = 0;
    int64_t limit = -1, rows = 0;
    int64_t file_lines = 0;     // integer tables: lines of the text handed out so far, blank and comment lines included
    int64_t chunks = 0;
    std::vector<char> carry;    // text not handed out yet: [carry_pos, size)
    size_t host_peak = 0;       // largest buffer allocated (the producer thread writes it; read after reader_text_stop or between chunks)
    size_t carry_pos = 0;
};

// ---- the compressed hand-over: the producer only READS whole members; the device inflates them ----------------------
struct CompPipe : ChunkQueue<CompChunk> {
    std::vector<CompChunk *> all;
    TextAllocator alloc;
    size_t text_cap = 0, max_members = 0;
    uint64_t file_off = 0;
    size_t pre_pos = 0, pre_end = 0;   // text the line-oriented calls had inflated already: [pre_pos, pre_end) of the reader's buffer
};

namespace {

// room for `want` bytes of text plus the pad; keeps data[0 .. len)
bool chunk_reserve(TextPipe *p, TextChunk *c, size_t want)
{
    if (c->data && want + TEXT_PAD <= c->cap) return true;
    // a multiple of 16: the ingest copies the text in whole 16-byte units, (len + TEXT_PAD) rounded up, which must not pass the buffer's end
    const size_t cap = (want + TEXT_PAD + 15) & ~(size_t)15;
    char *q = (char *)p->alloc.alloc(cap, p->alloc.user);
    if (!q) return false;
    if (c->len) memcpy(q, c->data, c->len);
    if (c->data) p->alloc.release(c->data, p->alloc.user);
    c->data = q;
    c->cap = cap;
    p->host_peak = std::max(p->host_peak, cap);
    return true;
}

// The non-blank lines of data[0 .. len) -- every line ends with a newline, or (at the end of the file) with the buffer.
// table: an integer table -- a line that starts with '#' is no row either (np.loadtxt), no names are kept, and lineno receives
// each listed line's index among all lines of the text; *all_lines their number.
void list_lines(const char *data, size_t len, int threads, std::vector<uint32_t> &begin, std::vector<uint32_t> &end, std::string &names,
                bool table = false, std::vector<uint32_t> *lineno = nullptr, int64_t *all_lines = nullptr)
{
    begin.clear();
    end.clear();
    names.clear();
    if (lineno) lineno->clear();
    if (all_lines) *all_lines = 0;
    if (len == 0) return;
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)threads, len >> 20));
    std::vector<std::vector<uint32_t>> nl(T), lb(T), le(T), ln(T);
    std::vector<std::string> nm(T);
    run_threads(T, [&](int t) {
        const size_t a = len * (size_t)t / (size_t)T, b = len * (size_t)(t + 1) / (size_t)T;
        for (const char *q = data + a, *e = data + b; q < e;) {
            q = (const char *)memchr(q, '\n', (size_t)(e - q));
            if (!q) break;
            nl[t].push_back((uint32_t)(q - data));
            ++q;
        }
    });
    // thread t lists the lines that END in its range; the first of them starts after the last newline before the range
    std::vector<size_t> start(T, 0);
    {
        size_t prev = 0;
        for (int t = 0; t < T; ++t) {
            start[t] = prev;
            if (!nl[t].empty()) prev = (size_t)nl[t].back() + 1;
        }
        if (prev < len) nl[T - 1].push_back((uint32_t)len);      // last line without a newline
    }
    std::vector<uint32_t> line0(T, 0);                           // lines that end before thread t's range
    for (int t = 1; t < T; ++t) line0[t] = line0[t - 1] + (uint32_t)nl[t - 1].size();
    if (all_lines) *all_lines = (int64_t)line0[T - 1] + (int64_t)nl[T - 1].size();
    run_threads(T, [&](int t) {
        size_t b = start[t];
        uint32_t number = line0[t];
        for (uint32_t stop : nl[t]) {
            const char *q = data + b, *e = data + stop;
            while (q < e && is_delim(*q)) ++q;
            if (q < e && !(table && *q == '#')) {                // blank lines are not rows
                lb[t].push_back((uint32_t)b);
                le[t].push_back(stop);
                if (table) {
                    ln[t].push_back(number);
                } else {
                    const char *x = q;
                    while (x < e && !is_delim(*x)) ++x;
                    nm[t].append(q, x);
                    nm[t].push_back('\n');
                }
            }
            b = (size_t)stop + 1;
            ++number;
        }
    });
    for (int t = 0; t < T; ++t) {
        begin.insert(begin.end(), lb[t].begin(), lb[t].end());
        end.insert(end.end(), le[t].begin(), le[t].end());
        names += nm[t];
        if (lineno) lineno->insert(lineno->end(), ln[t].begin(), ln[t].end());
    }
}

void text_producer(wgs_reader *r)
{
    TextPipe *p = r->pipe;
    for (;;) {
        TextChunk *c = nullptr;
        if (!p->take_free(c)) return;
        const double t0 = now_s();
        c->len = 0;
        const size_t pending0 = p->carry.size() - p->carry_pos;
        if (!chunk_reserve(p, c, std::max(p->chunk_bytes, std::min(pending0, p->chunk_bytes) + r->src.want_room()))) return p->fail(1, "out of (pinned) memory for the text buffers");
        size_t complete = 0;
        bool from_carry_only = false;
        for (;;) {
            // first what is pending from before (the partial line of the last chunk; at the start, everything the
            // line-oriented calls had already inflated), then the inflater
            if (p->carry_pos < p->carry.size()) {
                const size_t take = std::min(p->carry.size() - p->carry_pos, c->cap - TEXT_PAD - c->len);
                memcpy(c->data + c->len, p->carry.data() + p->carry_pos, take);
                c->len += take;
                p->carry_pos += take;
                if (p->carry_pos == p->carry.size()) {
                    p->carry.clear();
                    p->carry_pos = 0;
                }
            }
            from_carry_only = p->carry_pos > 0;              // pending text left: nothing was inflated into this chunk
            while (!from_carry_only && !r->eof) {
                const size_t room = c->cap - TEXT_PAD - c->len;
                if (room < r->src.min_room()) break;
                const bool batch = r->src.segmented;
                const long got = r->src.read(c->data + c->len, room);
                if (got == -2) break;
                if (got < 0) return p->fail(1, "read error while inflating the Beagle file");
                if (got == 0) {
                    r->eof = true;
                    break;
                }
                c->len += (size_t)got;
                if (batch) break;
            }
            const char *last = c->len ? (const char *)memrchr(c->data, '\n', c->len) : nullptr;
            if (r->eof && !from_carry_only) {
                complete = c->len;
                break;
            }
            if (last && (from_carry_only || c->cap - TEXT_PAD - c->len < r->src.min_room() || r->src.segmented || c->len >= p->chunk_bytes / 2)) {
                complete = (size_t)(last - c->data) + 1;
                break;
            }
            // one line longer than the buffer, or the next unit does not fit behind what is there: grow
            if (c->len + std::max(p->chunk_bytes, r->src.want_room()) >= (1ull << 32) - TEXT_PAD)
                return p->fail(1, "a Beagle line longer than 4 GiB");
            if (!chunk_reserve(p, c, c->len + std::max(p->chunk_bytes, r->src.want_room()))) return p->fail(1, "out of (pinned) memory for the text buffers");
        }
        if (from_carry_only) p->carry_pos -= c->len - complete;      // the cut-off tail is still there, right before carry_pos
        else p->carry.assign(c->data + complete, c->data + c->len);
        c->len = complete;
        memset(c->data + c->len, '\n', TEXT_PAD);
        const double t1 = now_s();
        int64_t all_lines = 0;
        list_lines(c->data, c->len, r->threads, c->begin, c->end, c->names, r->table, r->table ? &c->lineno : nullptr, &all_lines);
        c->first_line = p->file_lines;
        p->file_lines += all_lines;
        c->inflate_s = t1 - t0;
        c->scan_s = now_s() - t1;
        bool last_chunk = r->eof && p->carry.empty();
        c->first_row = p->rows;
        if (p->limit >= 0 && p->rows + (int64_t)c->begin.size() >= p->limit) {
            const size_t keep = (size_t)(p->limit - p->rows);
            if (keep < c->begin.size()) {
                c->begin.resize(keep);
                c->end.resize(keep);
                if (r->table) c->lineno.resize(keep);
                size_t at = 0;
                for (size_t i = 0; i < keep; ++i) at = c->names.find('\n', at) + 1;
                c->names.resize(at);
            }
            last_chunk = true;
        }
        p->rows += (int64_t)c->begin.size();
        p->chunks += c->begin.empty() ? 0 : 1;
        if (c->begin.empty()) p->recycle(c, last_chunk);     // nothing to hand over: back on the free list, unseen
        else p->publish(c, last_chunk);
        if (last_chunk) return;
    }
}

void comp_producer(wgs_reader *r)
{
    CompPipe *p = r->cpipe;
    const int fd = fileno(r->src.fp);
    for (;;) {
        CompChunk *c = nullptr;
        if (!p->take_free(c)) return;
        const double t0 = now_s();
        c->in_off.clear();
        c->in_len.clear();
        c->isize.clear();
        c->text_bytes = 0;
        c->len = 0;
        c->last = false;
        c->pre_text = nullptr;
        c->pre_len = 0;
        if (p->pre_pos < p->pre_end) {                                     // first what was inflated already, a chunk's worth at a time
            c->pre_text = r->buf.data() + p->pre_pos;
            c->pre_len = std::min(p->pre_end - p->pre_pos, p->text_cap);
            p->pre_pos += c->pre_len;
            p->publish(c, false);
            continue;
        }
        // The file in slices (all threads copy their share out of the page cache), whole members counted off as they arrive,
        // until the device's text buffer or this staging buffer is full; the slices shrink towards the end so that little
        // is read twice.
        size_t got = 0, at = 0;
        bool file_end = false, full = false, corrupt = false, partial = false;
        while (!full && !file_end && !corrupt && got < c->cap) {
            size_t slice = (size_t)64 << 20;
            if (at > 0 && c->text_bytes > 0) {
                const double per_text = (double)at / (double)c->text_bytes;
                const double est = (double)(p->text_cap - c->text_bytes) * per_text * 1.03 + 262144.0 - (double)(got - at);
                slice = (size_t)std::min<double>((double)slice, std::max<double>(est, (double)(1 << 20)));
            }
            slice = std::min(slice, c->cap - got);
            const size_t n = pread_slices(fd, c->comp + got, slice, p->file_off + got, r->threads);
            file_end = n < slice;
            got += n;
            partial = false;
            while (at < got) {
                BgzfBlock b;
                const Bgzf k = bgzf_member(c->comp + at, got - at, b);
                if (k == Bgzf::need_more) {                                    // a partial member: the next slice completes it
                    partial = true;
                    break;
                }
                if (k != Bgzf::member) {
                    corrupt = true;
                    break;
                }
                const uint32_t isz = b.isize;
                if (c->text_bytes + isz > p->text_cap || (p->max_members && isz && c->isize.size() >= p->max_members)) {
                    full = true;
                    break;
                }
                if (isz) {
                    c->in_off.push_back(at + b.hdr);
                    c->in_len.push_back(b.csize - b.hdr - 8);
                    c->isize.push_back(isz);
                }
                c->text_bytes += isz;
                at += b.csize;
            }
        }
        if (corrupt || (file_end && partial)) return p->fail(1, "read error in the BGZF file (corrupt or truncated member)");
        if (at == 0 && !file_end) return p->fail(1, "a BGZF member larger than the staging buffer");
        c->len = at;
        p->file_off += at;
        c->last = file_end && at == got;                                   // the file ended with this chunk's last member
        c->read_s = now_s() - t0;
        const bool last = c->last;                                         // (once published, the chunk is the consumer's)
        p->publish(c, last);
        if (last) return;
    }
}

}  // namespace

bool reader_text_is_bgzf(const wgs_reader *r) { return r && r->src.bgzf; }

int reader_text_start(wgs_reader *r, size_t chunk_bytes, int nbuf, TextAllocator a, int64_t limit_rows)
{
    if (!r || r->pipe || !a.alloc || !a.release || nbuf < 1) {
        wgs_set_error("bad argument");
        return 2;
    }
    TextPipe *p = new TextPipe();
    p->alloc = a;
    p->chunk_bytes = std::min<size_t>(std::max<size_t>(chunk_bytes, r->table ? 16u << 10 : 1u << 20), (size_t)2 << 30);
    p->limit = limit_rows;
    // what the line-oriented calls left in the reader's buffer comes first
    p->carry.assign(r->buf.data() + r->pos, r->buf.data() + r->len);
    r->pos = r->len = 0;
    for (int i = 0; i < nbuf; ++i) {
        TextChunk *c = new TextChunk();
        c->slot = i;
        p->all.push_back(c);
        p->free_q.push_back(c);
    }
    r->pipe = p;
    if (limit_rows == 0) p->finished = true;
    else p->th = std::thread(text_producer, r);
    return 0;
}

int reader_text_next(wgs_reader *r, TextChunk **out, double *waited_s)
{
    if (!r || !r->pipe || !out) {
        wgs_set_error("bad argument");
        return 2;
    }
    return r->pipe->next(out, waited_s);
}

void reader_text_release(wgs_reader *r, TextChunk *c)
{
    if (r && r->pipe && c) r->pipe->release(c);
}

void reader_text_stop(wgs_reader *r)
{
    TextPipe *p = r ? r->pipe : nullptr;
    if (!p) return;
    p->stop_and_join();
    r->lines_read += p->rows;
    r->text_chunks = p->chunks;
    r->host_peak = std::max(r->host_peak, p->host_peak);
    for (TextChunk *c : p->all) {
        if (c->data) p->alloc.release(c->data, p->alloc.user);
        delete c;
    }
    delete p;
    r->pipe = nullptr;
}

size_t reader_host_peak(const wgs_reader *r)
{
    size_t peak = std::max(r->host_peak, std::max(r->buf.size(), std::max(r->src.cbuf.size(), r->src.in.size())));
    if (r->pipe) peak = std::max(peak, r->pipe->host_peak);
    return peak;
}

int reader_comp_start(wgs_reader *r, size_t comp_bytes, size_t text_cap, int nbuf, TextAllocator a, size_t max_members)
{
    if (!r || r->pipe || r->cpipe || !r->src.bgzf || !a.alloc || !a.release || nbuf < 1) {
        wgs_set_error("bad argument");
        return 2;
    }
    CompPipe *p = new CompPipe();
    p->alloc = a;
    p->text_cap = std::max<size_t>(text_cap, r->table ? 65536u : 1u << 20);   // (a BGZF member holds up to 64 KiB of text)
    p->max_members = max_members;
    comp_bytes = std::max<size_t>(comp_bytes, 1u << 20);
    p->pre_pos = r->pos;
    p->pre_end = r->len;
    // what the block-parallel host path had read ahead but not inflated is read again from the file
    p->file_off = (uint64_t)ftello(r->src.fp) - (uint64_t)(r->src.clen - r->src.cpos);
    for (int i = 0; i < nbuf; ++i) {
        CompChunk *c = new CompChunk();
        c->comp = (unsigned char *)a.alloc(comp_bytes, a.user);
        c->cap = comp_bytes;
        r->host_peak = std::max(r->host_peak, comp_bytes);
        p->all.push_back(c);
        if (!c->comp) {
            for (CompChunk *x : p->all) {
                if (x->comp) a.release(x->comp, a.user);
                delete x;
            }
            delete p;
            wgs_set_error("out of (pinned) memory for the compressed staging buffers");
            return 1;
        }
        p->free_q.push_back(c);
    }
    r->cpipe = p;
    p->th = std::thread(comp_producer, r);
    return 0;
}

int reader_comp_next(wgs_reader *r, CompChunk **out, double *waited_s)
{
    if (!r || !r->cpipe || !out) {
        wgs_set_error("bad argument");
        return 2;
    }
    return r->cpipe->next(out, waited_s);
}

void reader_comp_release(wgs_reader *r, CompChunk *c)
{
    if (r && r->cpipe && c) r->cpipe->release(c);
}

void reader_comp_stop(wgs_reader *r)
{
    CompPipe *p = r ? r->cpipe : nullptr;
    if (!p) return;
    p->stop_and_join();
    for (CompChunk *c : p->all) {
        if (c->comp) p->alloc.release(c->comp, p->alloc.user);
        delete c;
    }
    delete p;
    r->cpipe = nullptr;
    r->pos = r->len = 0;               // the buffered text went to the device with the first chunk
    r->eof = true;
}

// compressed bytes from the first member not yet inflated to the end of the file (-1: unknown)
int64_t reader_comp_bytes_left(wgs_reader *r)
{
    if (!r || !r->src.fp) return -1;
    struct stat sb;
    if (fstat(fileno(r->src.fp), &sb) != 0) return -1;
    const int64_t at = (int64_t)ftello(r->src.fp) - (int64_t)(r->src.clen - r->src.cpos);
    return std::max<int64_t>(0, (int64_t)sb.st_size - at);
}

bool reader_inflate_member(const unsigned char *deflate, uint32_t in_len, uint32_t isize, unsigned char *out)
{
    BlockInflater inf;
    if (!inf.init()) return false;
    BgzfBlock b;
    b.off = 0;
    b.hdr = 0;
    b.csize = in_len + 8;
    b.isize = isize;
    return inf.run(deflate, b, out);
}
