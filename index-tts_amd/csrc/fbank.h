#pragma once
#include "../../include/idxtts.h"
#include "ctx.h"
#include "gemm.h"

namespace idxtts {

// Kaldi filter bank of features.kaldi_fbank for a ragged batch (w2v-BERT's extractor and CAMPPlus's input): the frames of all rows, packed
// one after another, go through two exact-fp32 GEMMs (windowed real DFT of frame_length taps, mel filters); a finishing kernel takes
// the log and normalises every mel bin over the row's own frames.
struct FbankModel : ModelBase {
  idxtts_fbank_config cfg;
  int nbins = 0, nbins4 = 0;
  LinearWeights dft;      // [fft_length][frame_length]: rows n <= fft/2: window * cos(2 pi n k / fft); rows fft/2 + n, 1 <= n < fft/2: -window * sin
  LinearWeights mel;      // [num_mel_bins][nbins4] (zero columns beyond nbins)

  explicit FbankModel(const idxtts_fbank_config& c) : cfg(c) {}
  bool accepts(const std::string& name) const override { return name == "window" || name == "mel_filters"; }
  int finalize(std::map<std::string, HostTensor>& t, DeviceArena& arena) override;
  int frames(int n) const { return n < cfg.frame_length ? 0 : 1 + (n - cfg.frame_length) / cfg.hop_length; }
  size_t workspace_bytes(const int* n_samples, int B) const;
  int forward(const float* audio, int ld_audio, const int* n_samples, int B, float scale, int mode, float* out, int T_out, void* ws,
              size_t ws_bytes, hipStream_t st);
};

// audioio.sinc_resample (torchaudio's polyphase sinc_interp_hann correlation) for a ragged batch of one rate pair; kt = kernel^T [taps][nw]
int resample_forward(const float* kt, int orig, int nw, int width, const float* x, int ldx, const int* lengths, int B, float* out, int ldo,
                     hipStream_t st);

}  // namespace idxtts
