// Stand-alone robustness run of the FLAC-in parser (matcha-tts-24k_amd/csrc/flac_parse.h) on host memory: for each stream given on
// the command line, the stream itself, every truncation, and single-byte mutations (three masks) at a stride, each parsed from a
// heap block of exactly its size into an output block of exactly its capacity.  It checks only that every call returns; build it
// with the host compiler and -fsanitize=address,undefined, which turn a read or write outside either block into a failure:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I matcha-tts-24k_amd/csrc tools/flac_parse_check.cpp -o flac_parse_check
//   ./flac_parse_check [--stride N] tests/golden/rfc9639_example1.flac tests/golden/flac_in/*.flac
// It is no pytest test, never runs on a GPU machine and is never loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flac_parse.h"

namespace fl = mtts_flac;

static long g_calls = 0, g_accepted = 0;

// One call on exact-size blocks: the bytes, `capacity` output words, max_block words of scratch
static int64_t run(const std::vector<uint8_t>& bytes, int64_t capacity, int max_block) {
    uint8_t* data = static_cast<uint8_t*>(std::malloc(bytes.size() ? bytes.size() : 1));
    int32_t* out = static_cast<int32_t*>(std::malloc(capacity ? capacity * sizeof(int32_t) : 1));
    int32_t* ch1 = static_cast<int32_t*>(std::malloc(max_block * sizeof(int32_t)));
    if (!bytes.empty()) std::memcpy(data, bytes.data(), bytes.size());
    fl::Info info;
    const int64_t n = fl::parse_stream(data, (int64_t)bytes.size(), max_block, out, capacity, ch1, info);
    std::free(ch1);
    std::free(out);
    std::free(data);
    ++g_calls;
    g_accepted += n >= 0;
    return n;
}

int main(int argc, char** argv) {
    size_t stride = 1;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--stride") && i + 1 < argc) stride = (size_t)std::atol(argv[++i]);
        else paths.push_back(argv[i]);
    }
    if (paths.empty() || stride < 1) {
        std::fprintf(stderr, "usage: flac_parse_check [--stride N] stream.flac ...\n");
        return 2;
    }
    for (const char* path : paths) {
        std::FILE* f = std::fopen(path, "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
        std::vector<uint8_t> bytes;
        uint8_t chunk[4096];
        for (size_t got; (got = std::fread(chunk, 1, sizeof chunk, f)) > 0;) bytes.insert(bytes.end(), chunk, chunk + got);
        std::fclose(f);
        const long before = g_calls;
        const int64_t whole = run(bytes, 1 << 16, fl::MAX_BLOCK);
        const int64_t capacity = whole > 0 ? whole : 64;     // exactly what the stream needs: one sample more would leave the block
        run(bytes, capacity, fl::MAX_BLOCK);
        run(bytes, capacity > 1 ? capacity - 1 : 0, fl::MAX_BLOCK);
        run(bytes, capacity, fl::MIN_MAX_BLOCK);
        for (size_t cut = 0; cut < bytes.size(); ++cut) run(std::vector<uint8_t>(bytes.begin(), bytes.begin() + cut), capacity, fl::MAX_BLOCK);
        const uint8_t masks[3] = {0x01, 0x80, 0xFF};
        for (size_t at = 0; at < bytes.size(); at += stride)
            for (uint8_t mask : masks) {
                std::vector<uint8_t> bad = bytes;
                bad[at] ^= mask;
                run(bad, capacity, fl::MAX_BLOCK);
            }
        std::printf("%s: %zu bytes, %lld samples, %ld calls returned\n", path, bytes.size(), (long long)whole, g_calls - before);
    }
    std::printf("flac_parse_check: %ld calls returned, %ld streams accepted, no read or write left its block\n", g_calls, g_accepted);
    return 0;
}
