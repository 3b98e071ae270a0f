// What the units of the streamed reader (reader.cpp, reader_index.cpp, reader_pipes.cpp) share: the reader itself, the
// small helpers all of them use, and the declarations by which one unit calls another.  Host code only.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "../../include/wgsassign_hip.h"
#include "../../include/wgsassign_hip_debug.h"
#include "gz_source.h"
#include "reader_text.h"

void wgs_set_error(const char *fmt, ...);

inline bool is_delim(char c) { return c == '\t' || c == ' ' || c == '\n' || c == '\r'; }

struct wgs_reader {
    GzSource src;
    std::vector<std::string> samples;
    int gl_cols = 0;   // GL columns in the header (3 per individual)
    int n_inds = 0;
    RawBuf<char> buf;
    size_t len = 0, pos = 0;
    size_t fill_cap = (size_t)-1;   // most bytes one fill() appends (BGZF, while a reader is opened: the header and the lines up to
                                    // the first row need kilobytes, and what is left in the buffer reaches the device ingest
                                    // as host-inflated text)
    bool eof = false;
    std::string chunk_sites;   // '\n'-joined site names of the last chunk
    int threads = 1;
    int64_t lines_read = 0;
    int64_t text_chunks = 0;           // chunks the last text hand-over produced
    bool table = false;                // an integer table (wgs_reader_open_table): no site-name column, '#' comments, no header to parse
    int table_cols = 0;                // columns of its first data line
    int64_t skip_lines = 0;            // header lines skipped when it was opened
    size_t host_peak = 0;              // largest single host buffer held for it (wgs_depth_ingest_stats)
    struct CompPipe *cpipe = nullptr;  // the compressed hand-over (reader_text.h: CompChunk), when started
    struct TextPipe *pipe = nullptr;   // the text hand-over to the device tokeniser (reader_text.h), when started
};

// ---- reader.cpp
void parse_header(const char *p, const char *hend, std::vector<std::string> &samples, int &gl_cols);

// ---- reader_index.cpp
struct BeagleIndex {
    uint64_t file_size = 0, mtime = 0;
    int64_t sites = 0;
    int32_t gl_cols = 0;
    std::vector<std::string> samples;
    std::vector<AccessPoint> points;
};
// Loads the index and checks that it still describes `path` (size, and modification time in nanoseconds).
bool index_matches_file(const char *index_path, const char *path, BeagleIndex &idx);
