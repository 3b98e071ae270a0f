// BGZF (bgzip, htslib -- what ANGSD writes): a series of gzip members of at most 64 KiB, each announcing its own
// compressed size in a 'BC' extra subfield and its uncompressed size in the trailer, so the blocks can be found
// without inflating anything and inflated independently, in parallel.  Here: the ONE walk over such members (in memory
// and in a file), the whole-member inflater, and the two helpers every unit of the streamed reader reads files with.
// Host code only.
#pragma once
#include <dlfcn.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <thread>
#include <vector>

template <typename F>
void run_threads(int T, F work)
{
    if (T <= 1) {
        work(0);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(work, t);
    for (auto &x : th) x.join();
}

// Buffer that grows without being zero-filled (std::vector's resize would touch every new page: 13 ms for the 64 MiB of
// compressed staging at every open on the GPU box, 30 ms elsewhere, a seventh of a whole device ingest of 5.4 GB of text).
template <typename C>
struct RawBuf {
    C *p = nullptr;
    size_t n = 0;
    ~RawBuf() { free(p); }
    RawBuf() = default;
    RawBuf(const RawBuf &) = delete;
    RawBuf &operator=(const RawBuf &) = delete;
    C *data() const { return p; }
    size_t size() const { return n; }
    bool resize(size_t want)             // never shrinks; false: out of memory, nothing changed
    {
        if (want <= n) return true;
        C *q = (C *)realloc(p, want);
        if (!q) return false;
        p = q;
        n = want;
        return true;
    }
};

// bytes [offset, offset + bytes) of the file into dst, its slices copied out of the page cache by up to `threads` threads
// (one fread of 32 MiB was a quarter of the whole pass on a 32-thread host).  Returns the contiguous bytes from the start:
// a short slice is the end of the file.
inline size_t pread_slices(int fd, unsigned char *dst, size_t bytes, uint64_t offset, int threads)
{
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)threads, bytes >> 20));
    std::vector<size_t> part(T, 0);
    run_threads(T, [&](int t) {
        const size_t a = bytes * (size_t)t / (size_t)T, b = bytes * (size_t)(t + 1) / (size_t)T;
        size_t done = 0;
        while (a + done < b) {
            const ssize_t k = pread(fd, dst + a + done, b - a - done, (off_t)(offset + a + done));
            if (k <= 0) break;
            done += (size_t)k;
        }
        part[t] = done;
    });
    size_t got = 0;
    for (int t = 0; t < T; ++t) {
        got += part[t];
        if (part[t] < bytes * (size_t)(t + 1) / (size_t)T - bytes * (size_t)t / (size_t)T) break;
    }
    return got;
}

struct BgzfBlock {
    uint64_t off = 0;       // file offset of the member
    uint32_t csize = 0;     // whole member, header and trailer included
    uint32_t hdr = 0;       // bytes before the deflate data
    uint32_t isize = 0;     // uncompressed bytes
    uint32_t unused = 0;    // (explicit padding: the part files of the split index pass hold these records verbatim)
};

// ---- the member walk ------------------------------------------------------------------------------------------------
enum class Bgzf { member, need_more, not_bgzf, corrupt };

// The member header at p (n bytes available) gives b.csize and b.hdr.
inline Bgzf bgzf_header(const unsigned char *p, size_t n, BgzfBlock &b)
{
    if (n < 12) return Bgzf::need_more;
    if (p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) return Bgzf::not_bgzf;
    const size_t xlen = p[10] | ((size_t)p[11] << 8);
    if (n < 12 + xlen) return Bgzf::need_more;
    for (size_t q = 12; q + 4 <= 12 + xlen;) {
        const size_t slen = p[q + 2] | ((size_t)p[q + 3] << 8);
        if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && q + 6 <= 12 + xlen) {
            if ((p[3] & ~4) != 0) return Bgzf::not_bgzf;      // names / comments / header CRC: not what bgzip writes
            b.hdr = (uint32_t)(12 + xlen);
            b.csize = (uint32_t)(p[q + 4] | ((size_t)p[q + 5] << 8)) + 1;
            return Bgzf::member;
        }
        q += 4 + slen;
    }
    return Bgzf::not_bgzf;
}

// The member's last four bytes give b.isize; then the sizes must fit each other and the format.
inline Bgzf bgzf_trailer(const unsigned char *tail, BgzfBlock &b)
{
    b.isize = tail[0] | ((uint32_t)tail[1] << 8) | ((uint32_t)tail[2] << 16) | ((uint32_t)tail[3] << 24);
    return b.isize > 65536 || b.csize < b.hdr + 8 ? Bgzf::corrupt : Bgzf::member;
}

// The member at p, of which n bytes are in memory.  b.off is the caller's.
inline Bgzf bgzf_member(const unsigned char *p, size_t n, BgzfBlock &b)
{
    const Bgzf k = bgzf_header(p, n, b);
    if (k != Bgzf::member) return k;
    if (b.csize > n) return Bgzf::need_more;
    return bgzf_trailer(p + b.csize - 4, b);
}

// The member at file offset `off`, hopping: `window` (at most 512) bytes of header and the trailer are read, nothing in
// between.  A member that would end past `limit` is corrupt (UINT64_MAX: the file's size is not known), and so is a header
// that the window or the file's end cuts short.  need_more: the file ends exactly at `off`.
inline Bgzf bgzf_member_at(int fd, uint64_t off, size_t window, uint64_t limit, BgzfBlock &b)
{
    unsigned char head[512], tail[4];
    const ssize_t got = pread(fd, head, window, (off_t)off);
    if (got == 0) return Bgzf::need_more;
    const Bgzf k = got > 0 ? bgzf_header(head, (size_t)got, b) : Bgzf::not_bgzf;
    if (k != Bgzf::member) return k == Bgzf::need_more ? Bgzf::corrupt : k;
    if (off + b.csize > limit || pread(fd, tail, 4, (off_t)(off + b.csize - 4)) != 4) return Bgzf::corrupt;
    b.off = off;
    return bgzf_trailer(tail, b);
}

// ---- inflate of whole members ---------------------------------------------------------------------------------------
// libdeflate does that 2-3x faster than zlib; this image ships its shared library (libdeflate.so.0, 1.10) without the
// header, hence the three prototypes and dlopen.  Without the library, or with WGSASSIGN_INFLATE=zlib: zlib's raw inflate.
// Neither checks the member's CRC32 (gzread does; a corrupt block that still inflates to ISIZE bytes would show up as
// unparsable text).
struct LibDeflate {
    void *(*alloc)() = nullptr;
    void (*release)(void *) = nullptr;
    int (*decompress)(void *, const void *, size_t, void *, size_t, size_t *) = nullptr;
    bool ok = false;
    LibDeflate()
    {
        const char *want = getenv("WGSASSIGN_INFLATE");
        if (want && strcmp(want, "zlib") == 0) return;
        void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc = reinterpret_cast<void *(*)()>(dlsym(h, "libdeflate_alloc_decompressor"));
        release = reinterpret_cast<void (*)(void *)>(dlsym(h, "libdeflate_free_decompressor"));
        decompress = reinterpret_cast<int (*)(void *, const void *, size_t, void *, size_t, size_t *)>(dlsym(h, "libdeflate_deflate_decompress"));
        ok = alloc && release && decompress;
    }
};
inline const LibDeflate &libdeflate()
{
    static const LibDeflate L;
    return L;
}

struct BlockInflater {
    z_stream z;
    bool z_live = false;
    void *ld = nullptr;
    BlockInflater() { memset(&z, 0, sizeof z); }
    BlockInflater(const BlockInflater &) = delete;
    BlockInflater &operator=(const BlockInflater &) = delete;
    ~BlockInflater()
    {
        if (ld) libdeflate().release(ld);
        if (z_live) inflateEnd(&z);
    }
    bool init()
    {
        if (libdeflate().ok && (ld = libdeflate().alloc()) != nullptr) return true;
        z_live = inflateInit2(&z, -15) == Z_OK;
        return z_live;
    }
    // one member (raw deflate between its header and trailer; `member` is its first byte) into out[0 .. isize)
    bool run(const unsigned char *member, const BgzfBlock &b, unsigned char *out)
    {
        if (b.isize == 0) return true;
        if (ld) return libdeflate().decompress(ld, member + b.hdr, b.csize - b.hdr - 8, out, b.isize, nullptr) == 0;
        if (inflateReset(&z) != Z_OK) return false;
        z.next_in = const_cast<unsigned char *>(member) + b.hdr;
        z.avail_in = b.csize - b.hdr - 8;
        z.next_out = out;
        z.avail_out = b.isize;
        return inflate(&z, Z_FINISH) == Z_STREAM_END && z.avail_out == 0;
    }
    // the block at b.off of the file: read into cb (room for a whole member), inflated into out
    bool run_at(int fd, const BgzfBlock &b, unsigned char *cb, unsigned char *out)
    {
        return pread(fd, cb, b.csize, (off_t)b.off) == (ssize_t)b.csize && run(cb, b, out);
    }
};
