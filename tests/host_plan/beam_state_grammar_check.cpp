// The readers' gate (csrc/beam_state.h) with BeamState::grammar, the flag casr_beam_grammar sets, as a
// program of its own under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_grammar_host_sanitizer.py builds and runs it): the flag defaults to false and then changes
// nothing; with it set the kind is BEAM_PLAIN or BEAM_LM, the readers that assume a casr_beam's tree and
// scores are refused as after a fused beam, the records stay readable, rec_lm is readable iff an LM took
// part, and the next beam entry clears the flag.
#include <stdio.h>
#include <stdlib.h>

#include "beam_state.h"

using namespace casr;

#define CHECK(c)                                                                        \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      fprintf(stderr, "beam_state_grammar_check: %s failed (line %d)\n", #c, __LINE__); \
      exit(2);                                                                          \
    }                                                                                   \
  } while (0)

// what casr_beam_grammar leaves (casr_capi.hip: beam_ran, then the flag)
static BeamState grammar_entry(bool with_lm, int k, float lmw, float lenw) {
  BeamState s{with_lm ? BEAM_LM : BEAM_PLAIN, k, lmw, lenw};
  s.grammar = true;
  return s;
}

int main() {
  // the default: off, and the table of every kind is what it was
  int pairs = 0;
  for (int kind = 0; kind < BEAM_KINDS; ++kind)
    for (int mbr = 0; mbr < 2; ++mbr)
      for (int reader = 0; reader < BEAM_READERS; ++reader) {
        BeamState s{kind, 4, 0.25f, 0.5f};
        s.mbr = mbr != 0;
        CHECK(!s.grammar);
        BeamState t = s;
        t.grammar = false;
        CHECK(beam_gate(s, reader) == beam_gate(t, reader));
        ++pairs;
      }
  CHECK(pairs == 5 * 2 * 8);
  const int assume_plain[] = {READ_RESCORE, READ_MBR, READ_NBEST, READ_CONFUSION};
  for (int with_lm = 0; with_lm < 2; ++with_lm) {
    const BeamState s = grammar_entry(with_lm != 0, 8, 1.5f, 0.5f);
    CHECK(s.kind == (with_lm ? BEAM_LM : BEAM_PLAIN) && s.k == 8 && !s.mbr && s.grammar);
    CHECK(beam_gate(s, READ_RECORDS) == GATE_OK);
    for (int reader : assume_plain) CHECK(beam_gate(s, reader) == GATE_AFTER_FUSED);
    CHECK(beam_gate(s, READ_MBR_DISTANCES) == GATE_BEFORE);
    CHECK(beam_gate(s, READ_RECORD_LM) == (with_lm ? GATE_OK : GATE_BEFORE));
    CHECK(beam_gate(s, READ_RECORD_BIAS) == GATE_BEFORE);
    CHECK(s.has_lm() == (with_lm != 0) && !s.has_bias());
  }
  // without the flag the same kinds read as a casr_beam and a casr_beam_lm do
  BeamState p{BEAM_PLAIN, 8, 0.f, 0.f};
  for (int reader : assume_plain) CHECK(beam_gate(p, reader) == GATE_OK);
  // the next beam entry assigns a fresh state: the flag is gone, the readers are back
  BeamState s = grammar_entry(false, 4, 0.f, 0.f);
  s = BeamState{BEAM_PLAIN, 4, 0.f, 0.f};
  CHECK(!s.grammar);
  for (int reader : assume_plain) CHECK(beam_gate(s, reader) == GATE_OK);
  // an encode spends a grammar beam as any other
  s = grammar_entry(true, 4, 0.f, 0.f);
  s = BeamState{};
  for (int reader = 0; reader < BEAM_READERS; ++reader) CHECK(beam_gate(s, reader) == GATE_BEFORE);
  printf("beam_state_grammar_check ok\n");
  return 0;
}
