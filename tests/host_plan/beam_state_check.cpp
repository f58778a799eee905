// The beam's state and its readers' gate (csrc/beam_state.h) on the host, as a program of its own under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_beam_state_host.py builds and runs it):
// every (kind, mbr) x reader pair against the table of include/casr.h's readers, written out here a
// second time, and the transitions the C API makes (casr_capi.hip: casr_encode, prepare_decode, beam_ran,
// casr_beam_mbr) replayed on a BeamState.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "beam_state.h"

using namespace casr;

#define CHECK(c)                                                                \
  do {                                                                          \
    if (!(c)) {                                                                 \
      fprintf(stderr, "beam_state_check: %s failed (line %d)\n", #c, __LINE__); \
      exit(2);                                                                  \
    }                                                                           \
  } while (0)

// the table, reader by reader, as DESIGN.md 3.3f states it
static int expected(int kind, bool mbr, int reader) {
  const bool none = kind == BEAM_NONE, plain = kind == BEAM_PLAIN;
  const bool lm = kind == BEAM_LM || kind == BEAM_BIAS_LM, bias = kind == BEAM_BIAS || kind == BEAM_BIAS_LM;
  switch (reader) {
    case READ_RECORDS: return none ? GATE_BEFORE : GATE_OK;
    case READ_RESCORE:
    case READ_MBR:
    case READ_NBEST:
    case READ_CONFUSION: return plain ? GATE_OK : none ? GATE_BEFORE : GATE_AFTER_FUSED;
    case READ_MBR_DISTANCES: return !none && mbr ? GATE_OK : GATE_BEFORE;
    case READ_RECORD_LM: return lm ? GATE_OK : GATE_BEFORE;
    default: return bias ? GATE_OK : GATE_BEFORE;  // READ_RECORD_BIAS
  }
}

// what the API does to the state
static void encode(BeamState& s) { s = BeamState{}; }
static void prepared(BeamState& s) { s = BeamState{}; }  // prepare_decode re-carves the workspaces
static void greedy_or_score(BeamState& s) { prepared(s); }
static void beam_entry(BeamState& s, int kind, int k, float lmw, float lenw) {
  prepared(s);
  s = BeamState{kind, k, lmw, lenw};
}
static bool beam_mbr(BeamState& s) {
  if (beam_gate(s, READ_MBR) != GATE_OK) return false;
  s.mbr = true;
  return true;
}

int main() {
  int pairs = 0;
  for (int kind = 0; kind < BEAM_KINDS; ++kind)
    for (int mbr = 0; mbr < 2; ++mbr)
      for (int reader = 0; reader < BEAM_READERS; ++reader) {
        BeamState s{kind, 4, 0.25f, 0.5f};
        s.mbr = mbr != 0;
        CHECK(beam_gate(s, reader) == expected(kind, s.mbr, reader));
        ++pairs;
      }
  CHECK(pairs == 5 * 2 * 8);
  // the names the refusals are built from
  const char* follows[BEAM_READERS] = {"casr_beam", "casr_beam", "casr_beam", "casr_beam", "casr_beam",
                                       "casr_beam_mbr", "casr_beam_lm", "casr_beam_bias"};
  for (int reader = 0; reader < BEAM_READERS; ++reader) {
    CHECK(strncmp(BEAM_READER_NAME[reader], "casr_beam_", 10) == 0);
    CHECK(strcmp(BEAM_READER_FOLLOWS[reader], follows[reader]) == 0);
  }
  CHECK(strcmp(BEAM_READER_NAME[READ_MBR_DISTANCES], "casr_beam_mbr_distances") == 0);

  // a fresh handle, and an encode: nothing to read
  BeamState s;
  for (int reader = 0; reader < BEAM_READERS; ++reader) CHECK(beam_gate(s, reader) == GATE_BEFORE);
  encode(s);
  CHECK(s.kind == BEAM_NONE && !s.mbr);
  // each beam entry: its kind, width and weights, mbr cleared (also after a casr_beam_mbr of the beam before)
  const int kinds[] = {BEAM_PLAIN, BEAM_LM, BEAM_BIAS, BEAM_BIAS_LM};
  for (int kind : kinds) {
    beam_entry(s, BEAM_PLAIN, 8, 0.f, 0.f);
    CHECK(beam_mbr(s) && s.mbr);
    CHECK(beam_gate(s, READ_MBR_DISTANCES) == GATE_OK);
    beam_entry(s, kind, 4, 0.25f, 0.5f);
    CHECK(s.kind == kind && s.k == 4 && s.lm_weight == 0.25f && s.length_weight == 0.5f && !s.mbr);
    CHECK(beam_gate(s, READ_RECORDS) == GATE_OK);
    CHECK(beam_gate(s, READ_MBR_DISTANCES) == GATE_BEFORE);
    CHECK(s.has_lm() == (kind == BEAM_LM || kind == BEAM_BIAS_LM));
    CHECK(s.has_bias() == (kind == BEAM_BIAS || kind == BEAM_BIAS_LM));
    // casr_beam_mbr is refused after a fused beam and leaves the state as it was
    CHECK(beam_mbr(s) == (kind == BEAM_PLAIN));
    CHECK(s.mbr == (kind == BEAM_PLAIN) && s.kind == kind);
    // casr_greedy or casr_score spends the beam, whatever it was
    greedy_or_score(s);
    CHECK(s.kind == BEAM_NONE && !s.mbr);
    for (int reader = 0; reader < BEAM_READERS; ++reader) CHECK(beam_gate(s, reader) == GATE_BEFORE);
  }
  // a new encode spends it too
  beam_entry(s, BEAM_PLAIN, 4, 0.f, 0.f);
  CHECK(beam_mbr(s));
  encode(s);
  for (int reader = 0; reader < BEAM_READERS; ++reader) CHECK(beam_gate(s, reader) == GATE_BEFORE);
  printf("beam_state_check ok (%d pairs)\n", pairs);
  return 0;
}
