// harness_io.h - the file plumbing of the host harnesses (tests/*_host_harness.cpp): each reads a case file and writes a result
// file, both flat little-endian arrays whose layout the harness's own header comment documents.  A short read or write ends the
// program with exit status 2, which tests/harness.py's run() reports with the message.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <vector>

static const char * harness_name = "harness";            // open_in_out sets it; it names the program in the messages below

template <class T>
static std::vector<T> rd(FILE * f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "%s: short read\n", harness_name); exit(2); }
    return v;
}
template <class T>
static void wr(FILE * f, const T * p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "%s: short write\n", harness_name); exit(2); }
}
template <class T>
static void wr(FILE * f, const std::vector<T> & v) { wr(f, v.data(), v.size()); }

// Opens the last two arguments as the case file and the result file; false, with the reason on stderr, when it cannot.
static bool open_in_out(int argc, char ** argv, const char * name, FILE ** fin, FILE ** fout) {
    harness_name = name;
    if (argc < 3) { fprintf(stderr, "usage: %s [mode] cases.bin results.bin\n", name); return false; }
    *fin = fopen(argv[argc - 2], "rb");
    *fout = fopen(argv[argc - 1], "wb");
    if (!*fin || !*fout) { fprintf(stderr, "%s: cannot open the files\n", name); return false; }
    return true;
}
