// count_input.h -- dsm_count's input, read in batches: one pattern per line, the line's first whitespace-separated token
// (so a reference or dsm_node tuple file "path entropy id:freq ..." can be fed in as it is); blank lines are skipped.  Host code
// only, without HIP, so that tests/native/count_input_check.cpp can check it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace dsm {

struct PatternBatch {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets{0};  // pattern p = bytes[offsets[p], offsets[p + 1])
    size_t size() const { return offsets.size() - 1; }
    void clear() { bytes.clear(); offsets.assign(1, 0); }
};

class PatternReader {
public:
    // read(buf, cap) -> bytes read, 0 at the end of the input, < 0 on an error
    using ReadFn = std::function<long(char*, size_t)>;
    explicit PatternReader(ReadFn read, size_t bufsize = 1u << 20) : read_(std::move(read)), buf_(bufsize ? bufsize : 1) {}

    // Clears b and fills it with the next patterns, until max_pat patterns or at least max_bytes bytes are in it.  Returns
    // false when b is empty: the input has ended (or failed: error()).
    bool next(PatternBatch& b, size_t max_pat, size_t max_bytes) {
        b.clear();
        while (state_ == TOKEN || (b.size() < max_pat && b.bytes.size() < max_bytes)) {  // (a token is never split)
            if (pos_ == len_) {
                if (eof_) break;
                const long r = read_(buf_.data(), buf_.size());
                if (r < 0) { error_ = true; eof_ = true; }
                else if (r == 0) eof_ = true;
                else { len_ = (size_t)r; pos_ = 0; }
                if (eof_) {
                    if (state_ == TOKEN) end_token(b);  // a last line without a newline
                    state_ = START;
                    break;
                }
            }
            const char ch = buf_[pos_++];
            const bool nl = ch == '\n';
            const bool ws = nl || ch == ' ' || ch == '\t' || ch == '\r' || ch == '\v' || ch == '\f';
            if (state_ == START) {
                if (!ws) { state_ = TOKEN; b.bytes.push_back((uint8_t)ch); }
            } else if (state_ == TOKEN) {
                if (ws) { end_token(b); state_ = nl ? START : REST; }
                else b.bytes.push_back((uint8_t)ch);
            } else if (nl) {
                state_ = START;
            }
        }
        return b.size() > 0;
    }
    bool error() const { return error_; }

private:
    enum State { START, TOKEN, REST };  // before the line's token, inside it, after it (up to the newline)
    void end_token(PatternBatch& b) { b.offsets.push_back(b.bytes.size()); }
    ReadFn read_;
    std::vector<char> buf_;
    size_t pos_ = 0, len_ = 0;
    bool eof_ = false, error_ = false;
    State state_ = START;
};

}  // namespace dsm
