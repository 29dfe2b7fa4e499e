// hole_bits.h — the host half of an index handle's hole bits (what a hole is, the device half and the protocol: HoleBits, api_types.inc.h):
// one bit per position, the number of set bits, the words changed since they were last taken.  Nothing of HIP: tests/cpp/test_hole_bits_cpu.cc.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct HoleWords {
  std::vector<uint64_t> words;
  uint64_t nholes = 0;             // set bits: set_range and clear keep it, nobody else writes it
  // words that span `rows` positions: the last position's word and one spare behind it, as both handles have always sized them
  static uint64_t words_for(uint64_t rows) { return (rows + 63) / 64 + 1; }
  bool is_hole(uint64_t pos) const { return (pos >> 6) < words.size() && ((words[pos >> 6] >> (pos & 63)) & 1ull); }
  // span `rows` positions: new words are zero (no hole), and it never shrinks
  void resize(uint64_t rows) { words.resize(std::max<size_t>(words.size(), (size_t)words_for(rows)), 0); }
  void set_range(uint64_t a, uint64_t b) {       // positions [a, b) become holes, word-wise; the words span b positions already (resize)
    if (a >= b) return;
    touch(a >> 6, (b - 1) >> 6);
    for (uint64_t w = a >> 6; w <= (b - 1) >> 6; ++w) {
      const uint64_t from = std::max(a, w << 6) & 63, cnt = std::min(b, (w + 1) << 6) - (w << 6) - from;      // bits [from, from + cnt) of word w
      const uint64_t mask = (cnt == 64 ? ~0ull : ((1ull << cnt) - 1)) << from;
      nholes += (uint64_t)__builtin_popcountll(mask & ~words[w]);      // (only the bits that were clear)
      words[w] |= mask;
    }
  }
  void clear(uint64_t pos) {                     // a hole becomes a row; any other position is left alone
    if (!is_hole(pos)) return;
    words[pos >> 6] &= ~(1ull << (pos & 63));
    nholes -= 1;
    touch(pos >> 6, pos >> 6);
  }
  bool take_dirty(uint64_t *lo, uint64_t *hi) {  // the words [*lo, *hi] changed since the last call (false: none); clean from now on
    *lo = dirty_lo; *hi = dirty_hi; dirty_lo = ~0ull; dirty_hi = 0;
    return *lo <= *hi;
  }

 private:
  uint64_t dirty_lo = ~0ull, dirty_hi = 0;       // lo > hi: nothing
  void touch(uint64_t lo, uint64_t hi) { dirty_lo = std::min(dirty_lo, lo); dirty_hi = std::max(dirty_hi, hi); }
};
