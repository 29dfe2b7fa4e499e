// The host half of the hole bits (zvec_amd/csrc/host/hole_bits.h) against a model that keeps one bit at a time: after every step the
// words, the count and is_hole agree, and the dirty range holds every word that changed and no word the step did not touch.
// Plain host C++, no GPU and no library: g++ tests/cpp/test_hole_bits_cpu.cc && ./a.out
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../zvec_amd/csrc/host/hole_bits.h"

namespace {

HoleWords hw;
std::vector<bool> model;       // one entry per position the words span
uint64_t model_count = 0;
int steps = 0;

#define REQUIRE(cond)                                                                          \
  do {                                                                                         \
    if (!(cond)) {                                                                             \
      fprintf(stderr, "step %d (%s): %s failed (%s:%d)\n", steps, what, #cond, __FILE__, __LINE__); \
      exit(1);                                                                                 \
    }                                                                                          \
  } while (0)

// `before`: the words as they were; [tlo, thi]: the words the step touched (tlo > thi: none)
void check(const char *what, const std::vector<uint64_t> &before, uint64_t tlo, uint64_t thi) {
  ++steps;
  REQUIRE(hw.words.size() * 64 == model.size());
  uint64_t bits = 0;
  for (size_t w = 0; w < hw.words.size(); ++w) {
    uint64_t expect = 0;
    for (unsigned b = 0; b < 64; ++b)
      if (model[w * 64 + b]) expect |= 1ull << b;
    REQUIRE(hw.words[w] == expect);
    bits += (uint64_t)__builtin_popcountll(expect);
  }
  REQUIRE(bits == model_count);
  REQUIRE(hw.nholes == model_count);
  for (uint64_t pos : {0ull, 1ull, 63ull, 64ull, 65ull, 127ull, 128ull, 129ull, 191ull, 192ull, (unsigned long long)model.size() - 1,
                       (unsigned long long)model.size(), (unsigned long long)model.size() + 64, 1ull << 40})
    REQUIRE(hw.is_hole(pos) == (pos < model.size() && model[pos]));
  uint64_t lo = 0, hi = 0;
  const bool dirty = hw.take_dirty(&lo, &hi);
  if (dirty) REQUIRE(tlo <= thi && lo >= tlo && hi <= thi);                  // within the words touched
  for (size_t w = 0; w < hw.words.size(); ++w) {
    const uint64_t was = w < before.size() ? before[w] : 0;                  // (a new word is zero: unchanged)
    if (hw.words[w] != was) REQUIRE(dirty && lo <= w && w <= hi);             // every changed word
  }
  REQUIRE(!hw.take_dirty(&lo, &hi));                                          // taken: clean until the next change
}

void resize(uint64_t rows) {
  const char *what = "resize";
  const std::vector<uint64_t> before = hw.words;
  hw.resize(rows);
  if (model.size() < HoleWords::words_for(rows) * 64) model.resize((size_t)HoleWords::words_for(rows) * 64, false);
  REQUIRE(hw.words.size() >= before.size());                                 // never shrinks
  check(what, before, 1, 0);
}

void set_range(uint64_t a, uint64_t b) {
  const std::vector<uint64_t> before = hw.words;
  hw.set_range(a, b);
  for (uint64_t p = a; p < b; ++p)
    if (!model[p]) { model[p] = true; ++model_count; }
  if (a < b) check("set_range", before, a >> 6, (b - 1) >> 6);
  else check("set_range (empty)", before, 1, 0);
}

void clear(uint64_t pos) {
  const std::vector<uint64_t> before = hw.words;
  hw.clear(pos);
  if (pos < model.size() && model[pos]) { model[pos] = false; --model_count; }
  check("clear", before, pos >> 6, pos >> 6);
}

}  // namespace

int main() {
  const char *what = "main";
  const uint64_t edges[] = {0, 63, 64, 65, 127, 128};
  REQUIRE(HoleWords::words_for(0) == 1 && HoleWords::words_for(1) == 2 && HoleWords::words_for(64) == 2 && HoleWords::words_for(65) == 3);
  clear(5);                                        // nothing is there yet: no word, no hole
  set_range(0, 0);
  resize(129);                                     // positions 0 .. 128 and the spare word: 4 words
  REQUIRE(hw.words.size() == 4);
  // every range that starts and ends on an edge: empty ones, single bits (63..64, 64..65, 127..128), whole words, two words; each
  // is set twice (the second time nothing is clear any more: the count must not move) and taken apart bit by bit, each bit twice
  for (uint64_t a : edges)
    for (uint64_t b : edges) {
      if (a > b) continue;
      set_range(a, b);
      const uint64_t had = hw.nholes;
      set_range(a, b);
      REQUIRE(hw.nholes == had && had == b - a);
      for (uint64_t p = a; p < b; ++p) {
        clear(p);
        clear(p);                                  // a clear bit: the count must not move
      }
      REQUIRE(hw.nholes == 0);
    }
  set_range(128, 129);                             // the last position alone
  set_range(60, 135);                              // three words
  resize(10);                                      // (fewer rows: nothing happens)
  REQUIRE(hw.words.size() == 4);
  resize(1000);                                    // a resize that adds words: zero, and the old bits stay
  REQUIRE(hw.words.size() == HoleWords::words_for(1000));
  set_range(60, 260);                              // overlaps what is set: five words, only the clear bits count
  set_range(191, 193);
  set_range(0, 1000);
  REQUIRE(hw.nholes == 1000);
  set_range(0, 1000);
  for (uint64_t p : {0ull, 63ull, 64ull, 65ull, 127ull, 128ull, 999ull, 1000ull, 5000ull}) clear(p);
  REQUIRE(hw.nholes == 993);
  // pseudo-random soak (fixed seed): ranges, clears and growth mixed
  uint64_t x = 88172645463325252ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int i = 0; i < 3000; ++i) {
    const uint64_t span = (hw.words.size() - 1) * 64;      // positions the words span, without the spare word
    const uint64_t r = rnd() % 16;
    if (r == 0) resize(span + rnd() % 200);
    else if (r < 8) { const uint64_t a = rnd() % span, len = rnd() % 4 ? rnd() % 70 : rnd() % 400; set_range(a, a + len < span ? a + len : span); }
    else clear(rnd() % (span + 100));
  }
  printf("hole bits: %d steps, %zu words, %llu holes at the end\nok\n", steps, hw.words.size(), (unsigned long long)hw.nholes);
  return 0;
}
