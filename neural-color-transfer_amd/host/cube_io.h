// cube_io.h — writer of .cube 3D look-up tables (the text format ffmpeg's lut3d, Resolve and Nuke read): "LUT_3D_SIZE N", then N^3 lines "R G B" with values in
// [0, 1] and red varying fastest. A table of the library (SPEC §6.6) is float [N][N][N][3] indexed [ib][ig][ir] with BGR channels in grey levels: its node order is
// the file's line order, the channels are turned round, every value is divided by 255 in fp32 and clamped. %.9g prints an fp32 value so that it reads back bit for bit.
#pragma once
#include <cstdio>
#include <string>

namespace cubeio {

inline float unit(float v) {
    const float u = v / 255.0f;
    return u < 0.0f ? 0.0f : (u > 1.0f ? 1.0f : u);                     // a NaN never gets here: the library's fit produces finite tables
}

inline bool write(const std::string& path, const float* lut, int N, std::string& err) {
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { err = "cannot open " + path; return false; }
    bool ok = fprintf(f, "LUT_3D_SIZE %d\n", N) > 0;
    const size_t n = (size_t)N * N * N;
    for (size_t i = 0; i < n && ok; ++i) ok = fprintf(f, "%.9g %.9g %.9g\n", (double)unit(lut[i * 3 + 2]), (double)unit(lut[i * 3 + 1]), (double)unit(lut[i * 3])) > 0;
    ok = (fclose(f) == 0) && ok;
    if (!ok) err = "write error on " + path;
    return ok;
}

// what -resume takes for a finished table: the header and at least N^3 lines behind it
inline bool looks_complete(const std::string& path, int N) {
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return false;
    int n = 0; size_t lines = 0;
    const bool head = fscanf(f, "LUT_3D_SIZE %d", &n) == 1 && n == N;
    for (int c; head && (c = fgetc(f)) != EOF;) lines += c == '\n';
    fclose(f);
    return head && lines >= (size_t)N * N * N + 1;
}

}  // namespace cubeio
