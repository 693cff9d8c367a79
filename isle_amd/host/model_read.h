// isle_amd/host/model_read.h — the reference's model readers, restated for the host: read_sparse_model (src/infer.cpp:125-208) and
// read_model (:8-76), one serial pass over the bytes.  This is the host statement of the rule the device loader
// (isle_hip_load_model_text, isle_amd/csrc/model_load.hip) implements, the way trainer_detail::weight_text states the writer's: where
// these functions throw, the device call fails, and where they return, the floats are the same bit for bit.
//
//   <weight>   <digits>[.<digits>], at least one digit; the digits before and after the point accumulated in FPTYPE (fp32) as
//              v *= 10; v += d, the value (float)((double)before + (double)after * std::pow(0.1, digits after the point)).
//              At most 64 bytes (a limit the reference does not have).
//   sparse     "<topic> <word> <weight>" per line, ids at most 18 digits, minus `base` inside [0, num_topics) x [0, vocab_size); fields
//              separated by runs of blanks or tabs, '\r' ignored everywhere, blank lines skipped, the last '\n' optional; the last line
//              naming a cell wins, cells nobody names are +0.
//   dense      one line per topic, vocab_size tokens each, num_topics non-blank lines; "nan" is the quiet NaN 0x7fc00000.
// Limits the reference does not have, both refused as "bad character": a sparse line of more than 4096 bytes, more than 64 consecutive
// '\r' in a dense text (no walk of the device parser is longer than these).
// Deviations from the reference: it asserts on a malformed line and only prints "Bad format" for a foreign character; both throw here,
// "line <n>: <kind>" with the 1-based line.  Errors of a whole line (field count, ids, token count) are met at its end.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace ISLE {
namespace model_read {

constexpr int MAX_TOKEN_BYTES = 64;
constexpr int MAX_ID_DIGITS = 18;
constexpr uint64_t MAX_SPARSE_LINE = 4096;  // bytes of a sparse line, its '\n' excluded
constexpr int MAX_CR_RUN = 64;              // consecutive '\r' in a dense text

inline std::vector<char> read_file(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open model file " + path);
  std::fseek(f, 0, SEEK_END);
  const long sz = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)sz);
  if (sz && std::fread(buf.data(), 1, (size_t)sz, f) != (size_t)sz) {
    std::fclose(f);
    throw std::runtime_error("short read on " + path);
  }
  std::fclose(f);
  return buf;
}

[[noreturn]] inline void fail(uint64_t line, const char* kind) { throw std::runtime_error("line " + std::to_string(line) + ": " + kind); }

// one weight token as it is read
struct Weight {
  float before = 0.f, after = 0.f;
  int after_digits = 0, digits = 0, bytes = 0;
  bool point = false;
  char head[3] = {0, 0, 0};
  const char* bad = nullptr;  // the first violation
  void push(char ch) {
    if (++bytes > MAX_TOKEN_BYTES) {
      if (!bad) bad = "token too long";
      return;
    }
    if (bytes <= 3) head[bytes - 1] = ch;
    if (ch >= '0' && ch <= '9') {
      // the product is rounded on its own whatever the target: a compiler that contracts (-march with FMA) must not fuse it
      if (!point) {
        volatile float shifted = before * 10;
        before = shifted + (float)(ch - '0');
      } else {
        volatile float shifted = after * 10;
        after = shifted + (float)(ch - '0');
        ++after_digits;
      }
      ++digits;
    } else if (ch == '.' && !point) {
      point = true;
    } else if (!bad) {
      bad = "bad character";
    }
  }
  bool is_nan() const { return bytes == 3 && head[0] == 'n' && head[1] == 'a' && head[2] == 'n'; }
  // null and the value, or the violation
  const char* finish(bool dense, float* out) const {
    if (dense && is_nan()) {
      const uint32_t bits = 0x7fc00000u;
      std::memcpy(out, &bits, sizeof(float));
      return nullptr;
    }
    if (bad) return bad;
    if (digits == 0) return "bad character";
    volatile double scaled = (double)after * std::pow(0.1, after_digits);  // rounded before the sum, as above
    *out = (float)((double)before + scaled);
    return nullptr;
  }
};

// model_by_word: vocab_size x num_topics, word-major (element (word, topic) at word * num_topics + topic), as the reference holds it
inline void read_sparse_model(const char* buf, uint64_t size, uint64_t num_topics, uint64_t vocab_size, unsigned base, std::vector<float>& model_by_word,
                              uint64_t* entries) {
  model_by_word.assign(vocab_size * num_topics, 0.f);
  uint64_t id[2] = {0, 0}, n = 0, line = 1;
  int id_digits[2] = {0, 0}, field = 0;
  bool was_ws = false, any = false;
  Weight w;
  auto end_of_line = [&]() {
    if (any) {
      if (field != 2) fail(line, "too few fields");
      float v = 0.f;
      if (const char* bad = w.finish(false, &v)) fail(line, bad);
      if (id[0] < base || id[1] < base || id[0] - base >= num_topics || id[1] - base >= vocab_size) fail(line, "id zero or out of range");
      model_by_word[num_topics * (id[1] - base) + (id[0] - base)] = v;
      ++n;
    }
    id[0] = id[1] = 0;
    id_digits[0] = id_digits[1] = field = 0;
    was_ws = any = false;
    w = Weight();
  };
  uint64_t line_bytes = 0;
  for (uint64_t i = 0; i < size; ++i) {
    const char ch = buf[i];
    if (ch == '\n') {
      end_of_line();
      ++line;
      line_bytes = 0;
      continue;
    }
    if (++line_bytes > MAX_SPARSE_LINE) fail(line, "bad character");
    if (ch == '\r') continue;
    if (ch == ' ' || ch == '\t') {
      was_ws = true;
      continue;
    }
    if (was_ws && any && ++field > 2) fail(line, "too many fields");
    was_ws = false;
    any = true;
    if (field < 2) {
      if (ch < '0' || ch > '9') fail(line, "bad character");
      if (++id_digits[field] > MAX_ID_DIGITS) fail(line, "id zero or out of range");
      id[field] = id[field] * 10 + (uint64_t)(ch - '0');
    } else {
      w.push(ch);
      if (w.bad) fail(line, w.bad);
    }
  }
  end_of_line();  // no trailing newline
  if (entries) *entries = n;
}

// model: vocab_size x num_topics, column-major (element (word, topic) at word + topic * vocab_size)
inline void read_dense_model(const char* buf, uint64_t size, uint64_t num_topics, uint64_t vocab_size, std::vector<float>& model) {
  model.assign(vocab_size * num_topics, 0.f);
  uint64_t line = 1, topic = 0, word = 0;
  bool in_token = false;
  Weight w;
  auto end_of_token = [&]() {
    if (!in_token) return;
    float v = 0.f;
    if (const char* bad = w.finish(true, &v)) fail(line, bad);
    if (word < vocab_size && topic < num_topics) model[word + topic * vocab_size] = v;
    ++word;
    in_token = false;
    w = Weight();
  };
  auto end_of_line = [&]() {
    end_of_token();
    if (word == 0) return;  // blank
    if (word != vocab_size) fail(line, "wrong token count");
    ++topic;
    word = 0;
  };
  int cr_run = 0;
  for (uint64_t i = 0; i < size; ++i) {
    const char ch = buf[i];
    if (ch == '\r') {
      if (++cr_run > MAX_CR_RUN) fail(line, "bad character");
      continue;
    }
    cr_run = 0;
    if (ch == '\n') {
      end_of_line();
      ++line;
    } else if (ch == ' ' || ch == '\t') {
      end_of_token();
    } else {
      in_token = true;
      w.push(ch);
      if (w.bytes > MAX_TOKEN_BYTES) fail(line, w.bad);  // (an earlier violation of the token, or its length)
    }
  }
  end_of_line();
  if (topic != num_topics) fail(size && buf[size - 1] == '\n' ? line - 1 : line, "wrong line count");
}

}  // namespace model_read
}  // namespace ISLE
