// gzip input of the streamed reader, serial and with random access.  Host code only.
#pragma once
#include <stdio.h>
#include <zlib.h>

#include <new>
#include <string>

#include "bgzf.h"

// ---- gzip input with random access ------------------------------------------------------------------
// A gzip stream can only be inflated from its start -- unless one keeps, for chosen deflate-block
// boundaries, the 32 KiB of output that precede them (the dictionary the next block may refer to).
// wgs_reader_build_index makes ONE inflate pass over the file, counting the data lines (sites) and
// recording such access points (every `span` bytes of output; at the start of a gzip member -- BGZF
// files have one per 64 KiB -- no dictionary is needed); a reader opened from the index starts at the
// access point before its first row, so a rank that owns a later SNP range no longer inflates the
// ranges before it.
constexpr size_t GZ_WIN = 32768;

struct AccessPoint {
    uint64_t in = 0;            // compressed offset of the first byte not yet consumed
    uint64_t out = 0;           // uncompressed offset
    int64_t lines_before = 0;   // non-blank lines (header included) completed before `out`
    uint8_t bits = 0;           // bits of byte in-1 that belong to the next block (0: byte aligned)
    uint8_t content = 0;        // the line in progress at `out` already holds a non-delimiter character
    uint8_t at_line_start = 0;  // `out` is the first byte of a line
    uint8_t member_start = 0;   // a gzip member header starts at `in` (no dictionary needed)
    std::vector<unsigned char> window;   // GZ_WIN bytes of output before `out` (empty at a member start)
};

struct GzSource {
    FILE *fp = nullptr;
    z_stream z;
    bool z_live = false, raw = false, eof = false;
    bool plain = false;              // not compressed at all (integer tables: wgs_reader_open_table); read() hands the file's bytes on
    std::vector<unsigned char> in;
    // BGZF mode
    bool bgzf = false;
    int threads = 1;
    RawBuf<unsigned char> cbuf;
    size_t clen = 0, cpos = 0;
    std::vector<BgzfBlock> batch;
    // segmented mode: a plain-gzip file read through its index -- the stretches between consecutive access points
    // are inflated independently, each from its own 32 KiB dictionary, `threads` at a time (BGZF blocks, megabytes long)
    bool segmented = false;
    std::string seg_path;
    std::vector<AccessPoint> segs;   // stretch i = output [segs[i].out, segs[i+1].out); the last point runs to the end
    size_t seg_next = 0;
    size_t in_bytes = 4u << 20;      // compressed staging buffer of the serial stream

    ~GzSource() { close(); }
    void close()
    {
        if (z_live) inflateEnd(&z);
        z_live = false;
        if (fp) fclose(fp);
        fp = nullptr;
    }
    bool refill()
    {
        if (z.avail_in != 0) return true;
        const size_t got = fread(in.data(), 1, in.size(), fp);
        z.next_in = in.data();
        z.avail_in = (unsigned)got;
        return got != 0;
    }
    // from the first byte (ap == nullptr) or from an access point
    bool open(const char *path, const AccessPoint *ap)
    {
        close();
        fp = fopen(path, "rb");
        if (!fp) return false;
        in.resize(in_bytes);
        memset(&z, 0, sizeof z);
        eof = false;
        raw = ap && !ap->member_start;
        if (inflateInit2(&z, raw ? -15 : 15 + 32) != Z_OK) return false;
        z_live = true;
        if (!ap) return true;
        if (fseeko(fp, (off_t)(ap->in - (ap->bits ? 1 : 0)), SEEK_SET) != 0) return false;
        if (ap->bits) {
            const int c = getc(fp);
            if (c == EOF) return false;
            if (inflatePrime(&z, ap->bits, c >> (8 - ap->bits)) != Z_OK) return false;
        }
        if (raw && inflateSetDictionary(&z, ap->window.data(), (unsigned)ap->window.size()) != Z_OK) return false;
        return true;
    }
    // After open() at the start of a member: switch to parallel block inflation if the file is BGZF from here on
    // (checked block by block as they are read; a non-BGZF member later is an error, such files do not exist).
    void try_bgzf(int nthreads, size_t cbuf_bytes = 64u << 20)
    {
        if (raw) return;
        const off_t here = ftello(fp);
        unsigned char head[64];
        const size_t got = fread(head, 1, sizeof head, fp);
        fseeko(fp, here, SEEK_SET);
        BgzfBlock first;
        if (bgzf_header(head, got, first) == Bgzf::member) {
            bgzf = true;
            threads = nthreads > 0 ? nthreads : 1;
            if (!cbuf.resize(cbuf_bytes)) throw std::bad_alloc();
            clen = cpos = 0;
        }
    }
    long read_bgzf(char *dst, size_t cap)
    {
        for (;;) {
            // whole members available in cbuf[cpos, clen) that fit into `cap`
            batch.clear();
            size_t p = cpos, out = 0;
            bool need_more = false;
            while (p < clen) {
                BgzfBlock b;
                const Bgzf k = bgzf_member(cbuf.data() + p, clen - p, b);
                if (k == Bgzf::need_more) {
                    need_more = true;
                    break;
                }
                if (k != Bgzf::member) return -1;
                if (out + b.isize > cap) break;
                b.off = p;
                batch.push_back(b);
                out += b.isize;
                p += b.csize;
            }
            if (!batch.empty()) {
                std::vector<size_t> ooff(batch.size());
                size_t acc = 0;
                for (size_t i = 0; i < batch.size(); ++i) ooff[i] = acc, acc += batch[i].isize;
                const int T = (int)std::min<size_t>((size_t)threads, batch.size());
                std::vector<char> ok(T, 1);
                run_threads(T, [&](int t) {
                    BlockInflater inf;
                    if (!inf.init()) {
                        ok[t] = 0;
                        return;
                    }
                    for (size_t i = (size_t)t; i < batch.size(); i += (size_t)T)
                        if (!inf.run(cbuf.data() + batch[i].off, batch[i], reinterpret_cast<unsigned char *>(dst) + ooff[i])) ok[t] = 0;
                });
                for (char c : ok)
                    if (!c) return -1;
                cpos = p;
                if (acc > 0) return (long)acc;
                continue;                            // only empty members (the BGZF end marker): look further
            }
            if (!need_more && p < clen) return -2;   // the next member does not fit into `cap`
            // refill the compressed staging buffer
            if (cpos > 0) {
                memmove(cbuf.data(), cbuf.data() + cpos, clen - cpos);
                clen -= cpos;
                cpos = 0;
            }
            const off_t at = ftello(fp);
            const size_t got = pread_slices(fileno(fp), cbuf.data() + clen, cbuf.size() - clen, (uint64_t)at, threads);
            fseeko(fp, at + (off_t)got, SEEK_SET);
            clen += got;
            if (got == 0) {
                eof = true;
                return clen == 0 ? 0 : -1;           // trailing bytes that are not a whole member
            }
        }
    }
    static constexpr size_t SEG_BATCH_MAX = 512u << 20;      // text inflated by one batch of stretches
    void use_segments(const char *path, std::vector<AccessPoint> points, int nthreads)
    {
        if (bgzf || points.size() < 2 || nthreads < 2) return;
        segmented = true;
        seg_path = path;
        segs = std::move(points);
        seg_next = 0;
        threads = nthreads;
    }
    size_t seg_len(size_t i) const { return (size_t)(segs[i + 1].out - segs[i].out); }
    // room the next read() needs at least / would like to have
    size_t min_room() const
    {
        if (bgzf) return 65536;
        if (segmented && seg_next + 1 < segs.size()) return std::max<size_t>(seg_len(seg_next), 1);
        return 1;
    }
    size_t want_room() const
    {
        if (!segmented) return min_room();
        size_t total = 0;
        for (size_t c = 0; c < (size_t)threads && seg_next + c + 1 < segs.size(); ++c) {
            if (c > 0 && total + seg_len(seg_next + c) > SEG_BATCH_MAX) break;
            total += seg_len(seg_next + c);
        }
        return std::max<size_t>(total, 1);
    }
    // -3: no whole stretch is left (the one after the last access point has no known end) -- the serial stream,
    // reopened at that point, takes over
    long read_segments(char *dst, size_t cap)
    {
        for (;;) {
            if (seg_next + 1 >= segs.size()) {
                segmented = false;
                const AccessPoint last = std::move(segs[seg_next]);
                segs.clear();
                return open(seg_path.c_str(), &last) ? -3 : -1;
            }
            size_t c = 0, total = 0;
            while (c < (size_t)threads && seg_next + c + 1 < segs.size()) {
                const size_t len = seg_len(seg_next + c);
                if (total + len > cap || (c > 0 && total + len > SEG_BATCH_MAX)) break;
                total += len;
                ++c;
            }
            if (c == 0) return -2;
            std::vector<size_t> ooff(c);
            for (size_t i = 0, acc = 0; i < c; ++i) ooff[i] = acc, acc += seg_len(seg_next + i);
            std::vector<char> ok(c, 1);
            run_threads((int)c, [&](int i) {
                GzSource s;
                s.in_bytes = 1u << 20;
                const size_t len = seg_len(seg_next + i);
                size_t got = 0;
                if (!s.open(seg_path.c_str(), &segs[seg_next + i])) ok[i] = 0;
                while (ok[i] && got < len) {
                    const long k = s.read(dst + ooff[i] + got, len - got);
                    if (k <= 0) ok[i] = 0;       // the file ends before the index says it does
                    else got += (size_t)k;
                }
            });
            for (char f : ok)
                if (!f) return -1;
            for (size_t i = 0; i < c; ++i) std::vector<unsigned char>().swap(segs[seg_next + i].window);   // done with it
            seg_next += c;
            if (total > 0) return (long)total;
        }
    }
    // up to `cap` bytes of output; 0 at the end of the file, -1 on a corrupt stream, -2: the next unit (BGZF block,
    // stretch between access points) does not fit into `cap`
    long read(char *dst, size_t cap)
    {
        if (segmented) {
            const long k = read_segments(dst, cap);
            if (k != -3) return k;
        }
        if (eof) return 0;
        if (bgzf) return read_bgzf(dst, cap);
        if (plain) {
            const size_t got = fread(dst, 1, std::min<size_t>(cap, 1u << 30), fp);
            if (got == 0) eof = true;
            return (long)got;
        }
        z.next_out = reinterpret_cast<unsigned char *>(dst);
        z.avail_out = (unsigned)std::min<size_t>(cap, 1u << 30);
        const unsigned want = z.avail_out;
        while (z.avail_out != 0) {
            if (!refill()) {
                eof = true;             // input exhausted (a truncated last member ends the data like gzread's EOF)
                break;
            }
            const int ret = inflate(&z, Z_NO_FLUSH);
            if (ret == Z_STREAM_END) {  // end of a gzip member: another one may follow (concatenated gzip, BGZF)
                if (raw) {              // raw inflate leaves the 8-byte CRC32 + ISIZE trailer in the input
                    for (int skip = 8; skip > 0;) {
                        if (!refill()) break;
                        const unsigned k = std::min<unsigned>((unsigned)skip, z.avail_in);
                        z.next_in += k;
                        z.avail_in -= k;
                        skip -= (int)k;
                    }
                    raw = false;
                }
                if (!refill()) {
                    eof = true;
                    break;
                }
                if (inflateReset2(&z, 15 + 32) != Z_OK) return -1;
            } else if (ret != Z_OK && ret != Z_BUF_ERROR) {
                return -1;
            }
        }
        return (long)(want - z.avail_out);
    }
};
