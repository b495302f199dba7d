// CPU check of csrc/count_input.h: dsm_count's batched pattern reader against a direct restatement (split the whole text into
// lines, take each line's first whitespace-separated token, drop blank lines), on random texts read through buffers of 1..97 bytes
// and reads that return fewer bytes than asked, in batches of random size.  Covers lines split across read buffers, tabs, blank and
// whitespace-only lines, CR LF endings and a last line without a newline.  usage: count_input_check <cases> <seed>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../dsm-framework_amd/csrc/count_input.h"

static std::vector<std::string> restate(const std::string& text) {
    std::vector<std::string> out;
    size_t i = 0;
    while (i < text.size()) {
        size_t j = text.find('\n', i);
        if (j == std::string::npos) j = text.size();
        const std::string line = text.substr(i, j - i);
        const char* ws = " \t\r\v\f";
        const size_t a = line.find_first_not_of(ws);
        if (a != std::string::npos) out.push_back(line.substr(a, line.find_first_of(ws, a) - a));
        i = j + 1;
    }
    return out;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 3000;
    std::mt19937_64 rng(argc > 2 ? atoll(argv[2]) : 1);
    const char alphabet[] = "ACGTN-acZ\0";  // ('\0' is a pattern byte like any other)
    const char* spaces[] = {" ", "\t", "  ", " \t ", "\r"};
    long tokens = 0;
    for (int it = 0; it < cases; ++it) {
        std::string text;
        const int lines = (int)(rng() % 60);
        for (int l = 0; l < lines; ++l) {
            const int kind = (int)(rng() % 10);
            if (kind == 0) { text += "\n"; continue; }                        // blank
            if (kind == 1) { text += spaces[rng() % 5]; text += "\n"; continue; }  // whitespace only
            if (kind == 2) text += spaces[rng() % 4];                          // leading whitespace
            const int len = 1 + (int)(rng() % (it % 3 == 0 ? 300 : 30));
            for (int k = 0; k < len; ++k) text.push_back(alphabet[rng() % 10]);
            if (rng() % 2) {                                                    // the rest of a tuple line
                text += spaces[rng() % 4];
                text += "1.234567 0:6\t1:9 2:17";
            }
            if (rng() % 6 == 0) text += "\r";
            if (l + 1 < lines || rng() % 2) text += "\n";                       // the last line may end without one
        }
        const std::vector<std::string> want = restate(text);
        size_t at = 0;
        const size_t bufsize = 1 + rng() % 97;
        const bool short_reads = rng() % 2;
        dsm::PatternReader rd([&](char* b, size_t cap) -> long {
            size_t n = cap < text.size() - at ? cap : text.size() - at;
            if (short_reads && n > 1) n = 1 + rng() % n;
            memcpy(b, text.data() + at, n);
            at += n;
            return (long)n;
        }, bufsize);
        std::vector<std::string> got;
        dsm::PatternBatch b;
        const size_t max_pat = 1 + rng() % 7, max_bytes = 1 + rng() % 200;
        while (rd.next(b, max_pat, max_bytes)) {
            if (b.offsets.size() != b.size() + 1 || b.offsets[0] != 0 || b.offsets.back() != b.bytes.size()) {
                fprintf(stderr, "case %d: malformed batch\n", it);
                return 1;
            }
            if (b.size() > max_pat || (b.size() > 1 && b.offsets[b.size() - 1] >= max_bytes)) {
                fprintf(stderr, "case %d: batch of %zu patterns, %zu bytes exceeds %zu / %zu\n", it, b.size(), b.bytes.size(), max_pat, max_bytes);
                return 1;
            }
            for (size_t p = 0; p < b.size(); ++p)
                got.emplace_back((const char*)b.bytes.data() + b.offsets[p], b.offsets[p + 1] - b.offsets[p]);
        }
        if (rd.error() || got != want) {
            fprintf(stderr, "case %d: %zu patterns read, %zu expected (buffer %zu)\n", it, got.size(), want.size(), bufsize);
            for (size_t k = 0; k < got.size() && k < want.size(); ++k)
                if (got[k] != want[k]) { fprintf(stderr, "  first difference at pattern %zu\n", k); break; }
            return 1;
        }
        tokens += (long)got.size();
    }
    // a failing read is reported, not taken for the end of the input
    dsm::PatternReader bad([](char*, size_t) -> long { return -1; });
    dsm::PatternBatch b;
    if (bad.next(b, 10, 10) || !bad.error()) { fprintf(stderr, "read error not reported\n"); return 1; }
    printf("count_input ok: %d texts, %ld patterns\n", cases, tokens);
    return 0;
}
