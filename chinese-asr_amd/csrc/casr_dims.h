// Dimensions of the deployed configuration (gpd.py), fixed at compile time so every tile loop
// unrolls.  casr_create rejects any other configuration (CASR_ERR_UNSUPPORTED).  Plain C++: read
// by the kernels and by the host-only decode plan (decode_plan.h) alike.
#pragma once

namespace casr {

constexpr int F = 80;     // n_mels
constexpr int D = 720;    // encoder input (3 ch x 3 frames x 80)
constexpr int H = 256;    // encoder hidden per direction
constexpr int C = 512;    // encoder output / context size (2H)
constexpr int HD = 512;   // decoder hidden
constexpr int E = 256;    // embedding
constexpr int A = 128;    // attention size
constexpr int KDEC = E + C + HD;  // 1280: decoder LSTM contraction [emb | ctx | h]
constexpr int KPROJ = C + HD;     // 1024: projection contraction [ctx | h]
constexpr int ST16 = C + HD + HD;  // offset of the s16 split words [ctx16 | h16] in a state row
constexpr int ST = ST16 + C + HD;  // 2560: per-row decoder state [ctx | h | c | ctx16 | h16]
constexpr int KMAX_BEAM = 16;

}  // namespace casr
