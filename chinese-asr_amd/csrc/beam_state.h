// What a handle knows about its last beam search, and which call may read it (include/casr.h: the
// casr_beam_* readers), once, as plain C++ that the host code (casr_capi.hip) and the sanitizer program
// (tests/host_plan/beam_state_check.cpp) both compile.  The kernels take BeamTree by value and read it by
// beam_tree.h's rules.
//
// A beam entry (casr_beam, casr_beam_lm, casr_beam_bias, casr_beam_grammar) leaves the beam tree and the finished records
// in the handle's decode workspaces.  BeamState says which entry that was; BeamTree is the read-only
// view of what it left, filled once by that entry; beam_gate is the one rule for who may read it.  The
// state goes back to BEAM_NONE wherever those workspaces are given to another decode: casr_encode and
// every prepared decode (casr_greedy, casr_score, the next beam entry, which then sets its own kind).
#pragma once
#include <stdint.h>

namespace casr {

enum { BEAM_NONE = 0, BEAM_PLAIN, BEAM_LM, BEAM_BIAS, BEAM_BIAS_LM, BEAM_KINDS };

// (a beam entry leaves BeamState{kind, k, lm_weight, length_weight}: no MBR distances yet)
struct BeamState {
  int kind = BEAM_NONE;
  int k = 0;
  float lm_weight = 0.f, length_weight = 0.f;  // the beam's own (the readers' unfinished fallback)
  bool mbr = false;                            // casr_beam_mbr's distances of this beam are present
  bool grammar = false;  // casr_beam_grammar ran it (kind BEAM_PLAIN or BEAM_LM): the tree has dead rows
  bool has_lm() const { return kind == BEAM_LM || kind == BEAM_BIAS_LM; }      // lmws holds rec_lm
  bool has_bias() const { return kind == BEAM_BIAS || kind == BEAM_BIAS_LM; }  // biasws holds rec_full
};

enum {
  READ_RECORDS = 0, READ_RESCORE, READ_MBR, READ_NBEST, READ_CONFUSION, READ_MBR_DISTANCES, READ_RECORD_LM,
  READ_RECORD_BIAS, BEAM_READERS
};
// the reader's name and the call it must follow
constexpr const char* BEAM_READER_NAME[BEAM_READERS] = {
    "casr_beam_records", "casr_beam_rescore", "casr_beam_mbr", "casr_beam_nbest", "casr_beam_confusion",
    "casr_beam_mbr_distances", "casr_beam_record_lm", "casr_beam_record_bias"};
constexpr const char* BEAM_READER_FOLLOWS[BEAM_READERS] = {
    "casr_beam", "casr_beam", "casr_beam", "casr_beam", "casr_beam", "casr_beam_mbr", "casr_beam_lm", "casr_beam_bias"};

// GATE_BEFORE: "<reader> before <the call it must follow>"; GATE_AFTER_FUSED: the reader assumes the
// scores of a casr_beam and the last beam was casr_beam_lm, casr_beam_bias or casr_beam_grammar.  Both are
// CASR_ERR_STATE.
enum { GATE_OK = 0, GATE_BEFORE, GATE_AFTER_FUSED };

inline int beam_gate(const BeamState& s, int reader) {
  switch (reader) {
    case READ_RECORDS: return s.kind != BEAM_NONE ? GATE_OK : GATE_BEFORE;
    case READ_RESCORE:
    case READ_MBR:
    case READ_NBEST:
    case READ_CONFUSION:
      return s.kind == BEAM_NONE ? GATE_BEFORE : s.kind == BEAM_PLAIN && !s.grammar ? GATE_OK : GATE_AFTER_FUSED;
    case READ_MBR_DISTANCES: return s.kind != BEAM_NONE && s.mbr ? GATE_OK : GATE_BEFORE;
    case READ_RECORD_LM: return s.has_lm() ? GATE_OK : GATE_BEFORE;
    case READ_RECORD_BIAS: return s.has_bias() ? GATE_OK : GATE_BEFORE;
    default: return GATE_BEFORE;
  }
}

// What a reader needs of the beam that ran: its dimensions, the tree, the records, the final scores
// and the guard word.  Device pointers into the handle's decode workspaces, valid while the state is
// not BEAM_NONE.
struct BeamTree {
  int B = 0, k = 0, L = 0, V = 0;
  const int32_t* bp = nullptr;         // [L][B k]
  const int32_t* tk = nullptr;         // [L][B k]
  const int32_t* newdone = nullptr;    // [L]
  const float* rec_score = nullptr;    // [B][L][k]
  const int32_t* rec_src = nullptr;    // [B][L][k]
  const uint8_t* rec_valid = nullptr;  // [B][L][k]
  const float* score[2] = {};          // [B k] ping-pong: the executed steps' parity picks the final one
  int32_t* err = nullptr;              // the decode guard word
};

}  // namespace casr
