// Where the arrays of a synchronous host-buffer call (the *_host entries) lie
// in the model's staging buffer and its pinned mirror: the inputs first, in
// the order they were registered, so that one transfer sends them; the outputs
// after them, so that one transfer brings them back.  A NULL array takes no
// space.  Offsets count 8-byte words: an int32 array of B elements occupies
// (B + 1) / 2 of them, so every double array stays 8-byte aligned, and only
// its 4 B bytes are copied to the caller.  Pure integer logic without a HIP
// include (api.cpp: HostStage does the copies;
// tools/host_staging_host_test.cpp runs the rules with the host compiler).
#pragma once
#include <cstdint>

namespace drc_amd {

struct StagingLayout {
  static constexpr int kMaxArrays = 16;  // drc_qpid_stages_host: 6 inputs + 9 outputs
  struct Region {
    int64_t off;    // words from the start of the inputs / of the outputs
    int64_t bytes;  // what the caller's array holds (elements * element size)
    bool out;
  };
  Region r[kMaxArrays];
  int n = 0;
  int64_t in_words = 0, out_words = 0;

  // Registers one array of `count` elements of `elem_bytes` (4 or 8) each.
  // Returns its region, kNull for an array that is not there (`present`
  // false), kFull when kMaxArrays regions are taken.
  static constexpr int kNull = -1, kFull = -2;
  int add(bool present, bool out, int64_t count, int elem_bytes) {
    if (!present) return kNull;
    if (n == kMaxArrays) return kFull;
    int64_t& end = out ? out_words : in_words;
    r[n] = {end, count * elem_bytes, out};
    end += (count * elem_bytes + 7) / 8;
    return n++;
  }
  // Words from the start of the buffer (valid once every input is registered)
  int64_t offset(int i) const { return r[i].out ? in_words + r[i].off : r[i].off; }
  int64_t total_words() const { return in_words + out_words; }
};

}  // namespace drc_amd
