// The front-end of the prompt block on MI355X: Kaldi filter-bank features and the polyphase sinc resampler, for a ragged batch of
// prompts (the host numpy these restate: indextts_amd/features.py, indextts_amd/audioio.py).
//
// Reference: SeamlessM4TFeatureExtractor (transformers, feature_extraction_seamless_m4t.py: spectrogram(..., preemphasis=0.97,
//            remove_dc_offset=True, mel_floor=2^-23, log_mel="log"), per-bin normalisation, stride-2 stacking)      infer_v2.py:633, 680
//            torchaudio.compliance.kaldi.fbank(num_mel_bins=80, dither=0) minus its mean over time                 infer_v2.py:641-646
//            torchaudio.transforms.Resample (functional.py::_apply_sinc_resample_kernel)                            infer_v2.py:629-630
//
// Shaped as audio.hip: a framing kernel (mean removal and pre-emphasis, one wave per frame), the DFT as a GEMM against a matrix with the
// window folded in (the pre-emphasis runs before the window, so the fold is legal, and K is the frame length, not the FFT length),
// power, the mel GEMM, then one finishing kernel (floor, log, per-bin statistics over the row's own frames, in the host's order).  The frames of all rows are
// packed one after another, so the GEMMs see no padding.  Both GEMMs are lin_exact: split-bf16's 2^-16 of a frame's peak is not small in
// the quiet bins of a log power spectrum, and a prompt's features must not depend on which other prompts share its batch.
// Host lengths travel as kernel arguments (FB_ROWS rows per launch): no copy, no synchronisation, nothing a graph capture refuses.
#include <algorithm>
#include <cmath>

#include "device_util.h"
#include "fbank.h"
#include "model_util.h"

namespace idxtts {

int FbankModel::finalize(std::map<std::string, HostTensor>& t, DeviceArena& arena) {
  const int L = cfg.frame_length, F = cfg.fft_length, C = cfg.num_mel_bins;
  IDX_CHECK(L >= 4 && (L & 3) == 0 && F >= L && (F & 3) == 0 && cfg.hop_length > 0 && C > 0 && C <= 256, "filter bank shape");
  nbins = F / 2 + 1;
  nbins4 = (nbins + 3) & ~3;
  HostTensor *wd = nullptr, *mf = nullptr;
  if (need(t, "window", {L}, &wd) || need(t, "mel_filters", {C, nbins}, &mf)) return 1;
  // the imaginary parts of bins 0 and fft/2 are zero: fft_length output columns instead of 2 * nbins
  std::vector<float> m((size_t)F * L);
  const double w0 = 2.0 * M_PI / F;
  for (int n = 0; n < nbins; ++n)
    for (int k = 0; k < L; ++k) {
      const double ang = w0 * (double)(((long long)n * k) % F);
      m[(size_t)n * L + k] = (float)(wd->data[k] * std::cos(ang));
      if (n >= 1 && n < F / 2) m[(size_t)(F / 2 + n) * L + k] = (float)(-(double)wd->data[k] * std::sin(ang));
    }
  if (make_linear(arena, m.data(), nullptr, F, L, {WP16_NONE}, &dft)) return 1;
  return make_linear(arena, mf->data.data(), nullptr, C, nbins, {WP16_NONE, W_NK, nbins4}, &mel);
}

namespace {

constexpr int FB_ROWS = 32;      // rows per launch of the ragged kernels: their lengths are kernel arguments
struct FbRows {
  int frames[FB_ROWS];           // frames of the row
  int first[FB_ROWS];            // index of its first frame among the packed frames of the whole batch
};

struct FbBuf { float *fr, *spec, *pw, *mel; size_t bytes; };

FbBuf carve_fbank(const FbankModel& m, void* ws, size_t M) {
  FbBuf b;
  Carver k(ws);
  b.fr = k.take<float>(M * m.cfg.frame_length);
  b.spec = k.take<float>(M * m.cfg.fft_length);
  b.pw = k.take<float>(M * m.nbins4);
  b.mel = k.take<float>(M * m.cfg.num_mel_bins);
  b.bytes = (k.off + 255) & ~(size_t)255;
  return b;
}

// One wave per frame: fr = scale * audio[t * hop .. + L) minus its mean; out[0] = fr[0] * (1 - pre), out[i] = fr[i] - pre * fr[i - 1].
// grid (ceil(longest row's frames / 4), rows)
__global__ __launch_bounds__(256) void fbank_frame_kernel(float* fr, const float* audio, FbRows rows, int ld_audio, int L, int hop, float scale,
                                                          float pre) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= rows.frames[b]) return;      // the whole wave
  const float* a = audio + (size_t)b * ld_audio + (size_t)t * hop;
  float s = 0.0f;
  for (int i = lane; i < L; i += 64) s += a[i] * scale;
  const float mean = wave_sum(s) / (float)L;
  float* o = fr + ((size_t)rows.first[b] + t) * L;
  for (int i = lane; i < L; i += 64) {
    const float v = a[i] * scale - mean;
    o[i] = i ? v - pre * (a[i - 1] * scale - mean) : v * (1.0f - pre);
  }
}

// pw[m][n] = re[n]^2 + im[n]^2 (spec[m]: re of bins 0 .. F/2, then im of bins 1 .. F/2 - 1), zero in the columns that pad nbins to nbins4
__global__ __launch_bounds__(256) void fbank_power_kernel(float* pw, const float* spec, int F, int nbins4) {
  const size_t m = blockIdx.x;
  const float* re = spec + m * F;
  const float* im = re + F / 2;      // im[n], 1 <= n < F/2
  for (int n = threadIdx.x; n < nbins4; n += 256) {
    float p = 0.0f;
    if (n <= F / 2) {
      p = re[n] * re[n];
      if (n >= 1 && n < F / 2) p += im[n] * im[n];
    }
    pw[m * nbins4 + n] = p;
  }
}

// One workgroup per row: log(max(., floor)) of the row's frames in place, then every mel bin's statistics over those frames, then the
// output -- zero behind the row's frames.  The statistics are the host's, in the host's ORDER: numpy reduces the frame axis of a float32
// [T][C] array by adding the frames one after another, and at a stationary bin (a steady tone: values near 20 that move by 0.02) the
// rounding of that running sum is 4e-4 of the normalised feature -- any other order, a more accurate one too, differs from the
// reference by that much.  So thread c adds bin c's frames in order (reads coalesced over c; the loads do not depend on the sum), and
// the variance is the two-pass one with the product rounded before it is added, as numpy's.  E[x^2] - mean^2 would cancel here.
// `out` row b: [Tpad][C]; the w2v-BERT form's [T_out][2C] is the same memory with Tpad = 2 * T_out.      grid (rows), C <= FB_MAXC
constexpr int FB_MAXC = 256;
__global__ __launch_bounds__(256) void fbank_finish_kernel(float* out, float* mel, FbRows rows, int C, int Tpad, float floor_, int mode) {
  __shared__ float s_mean[FB_MAXC], s_sd[FB_MAXC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = rows.frames[b];
  float* x = mel + (size_t)rows.first[b] * C;
  for (int i = tid; i < T * C; i += 256) x[i] = logf(fmaxf(x[i], floor_));
  __syncthreads();
  if (tid < C) {
    float mean = 0.0f, sd = 1.0f;
    if (mode != IDXTTS_FBANK_RAW) {
      float s = x[tid];
#pragma unroll 8
      for (int f = 1; f < T; ++f) s += x[(size_t)f * C + tid];
      mean = s / (float)T;
    }
    if (mode == IDXTTS_FBANK_W2VBERT) {
      float d = x[tid] - mean;
      float q = __fmul_rn(d, d);
#pragma unroll 8
      for (int f = 1; f < T; ++f) {
        d = x[(size_t)f * C + tid] - mean;
        q += __fmul_rn(d, d);
      }
      sd = sqrtf(q / (float)(T - 1) + 1e-7f);
    }
    s_mean[tid] = mean;
    s_sd[tid] = sd;
  }
  __syncthreads();
  float* o = out + (size_t)b * Tpad * C;
  for (int i = tid; i < Tpad * C; i += 256) {
    const int f = i / C, c = i - f * C;
    float v = 0.0f;
    if (f < T) {
      v = x[i] - s_mean[c];
      if (mode == IDXTTS_FBANK_W2VBERT) v /= s_sd[c];
    }
    o[i] = v;
  }
}

size_t total_frames(const FbankModel& m, const int* n, int B) {
  size_t M = 0;
  for (int b = 0; b < B; ++b) M += (size_t)m.frames(n[b]);
  return M;
}

}  // namespace

size_t FbankModel::workspace_bytes(const int* n_samples, int B) const { return carve_fbank(*this, nullptr, total_frames(*this, n_samples, B)).bytes; }

int FbankModel::forward(const float* audio, int ld_audio, const int* n_samples, int B, float scale, int mode, float* out, int T_out, void* ws,
                        size_t ws_bytes, hipStream_t st) {
  IDX_CHECK(audio && out && n_samples, "null pointer");
  IDX_CHECK(B > 0, "shape");
  IDX_CHECK(mode == IDXTTS_FBANK_RAW || mode == IDXTTS_FBANK_CAMPPLUS || mode == IDXTTS_FBANK_W2VBERT, "mode");
  const int L = cfg.frame_length, F = cfg.fft_length, C = cfg.num_mel_bins;
  int Tmax = 0;
  for (int b = 0; b < B; ++b) {
    IDX_CHECK(n_samples[b] <= ld_audio, "a row is longer than ld_audio");
    const int T = frames(n_samples[b]);
    IDX_CHECK(T >= 1, "audio shorter than one frame");
    IDX_CHECK(mode != IDXTTS_FBANK_W2VBERT || T >= 2, "the audio is shorter than two frames");
    Tmax = std::max(Tmax, T);
  }
  const int Tpad = mode == IDXTTS_FBANK_W2VBERT ? 2 * T_out : T_out;
  IDX_CHECK(Tpad >= Tmax, "T_out is shorter than the longest row");
  IDX_CHECK((long long)Tpad * C < (1ll << 31), "T_out too long");
  const size_t M = total_frames(*this, n_samples, B);
  IDX_CHECK(M < (1u << 30), "too many frames");
  IDX_CHECK(ws && ws_bytes >= carve_fbank(*this, nullptr, M).bytes, "workspace too small");
  FbBuf w = carve_fbank(*this, ws, M);
  std::vector<FbRows> tabs(cdiv(B, FB_ROWS));
  int first = 0;
  for (int b = 0; b < B; ++b) {
    FbRows& r = tabs[b / FB_ROWS];
    r.frames[b % FB_ROWS] = frames(n_samples[b]);
    r.first[b % FB_ROWS] = first;
    first += r.frames[b % FB_ROWS];
  }
  for (int b0 = 0; b0 < B; b0 += FB_ROWS) {
    const int nb = std::min(FB_ROWS, B - b0);
    hipLaunchKernelGGL(fbank_frame_kernel, dim3(cdiv(Tmax, 4), nb), dim3(256), 0, st, w.fr, audio + (size_t)b0 * ld_audio, tabs[b0 / FB_ROWS],
                       ld_audio, L, cfg.hop_length, scale, cfg.preemphasis);
    IDX_LAUNCH_CHECK();
  }
  if (lin_exact(dft, w.fr, L, w.spec, F, (int)M, st)) return 1;
  hipLaunchKernelGGL(fbank_power_kernel, dim3((unsigned)M), dim3(256), 0, st, w.pw, w.spec, F, nbins4);
  IDX_LAUNCH_CHECK();
  if (lin_exact(mel, w.pw, nbins4, w.mel, C, (int)M, st)) return 1;
  for (int b0 = 0; b0 < B; b0 += FB_ROWS) {
    const int nb = std::min(FB_ROWS, B - b0);
    hipLaunchKernelGGL(fbank_finish_kernel, dim3(nb), dim3(256), 0, st, out + (size_t)b0 * Tpad * C, w.mel, tabs[b0 / FB_ROWS], C,
                       Tpad, 1.192092955078125e-07f, mode);
    IDX_LAUNCH_CHECK();
  }
  return 0;
}

namespace {

constexpr int RS_ROWS = 32, RS_TILE = 256;
struct RsRows { int len[RS_ROWS]; };

// out[b][o], o = f * nw + p: sum_t padded_b[f * orig + t] * kt[t][p].  A workgroup takes RS_TILE consecutive outputs of one row and stages
// the input samples they read in LDS (the implicit zero padding is applied there); consecutive lanes are consecutive phases p of the
// transposed table (coalesced) and read one LDS address per frame (broadcast).  The products are exact in float64 and are summed there, one
// rounding at the end: the result is the float32 nearest to the exact sum, whatever the order.      grid (ceil(ldo / RS_TILE), rows)
__global__ __launch_bounds__(RS_TILE) void resample_kernel(float* out, const float* x, const float* kt, RsRows rows, int ldx, int ldo, int orig,
                                                           int nw, int width, int taps) {
  extern __shared__ float xs[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int len = rows.len[b];
  const int target = (int)(((long long)nw * len + orig - 1) / orig);
  const int o0 = blockIdx.x * RS_TILE, o = o0 + tid;
  float* orow = out + (size_t)b * ldo;
  if (o0 >= target) {      // the whole workgroup
    if (o < ldo) orow[o] = 0.0f;
    return;
  }
  const int f_lo = o0 / nw, f_hi = (min(o0 + RS_TILE, target) - 1) / nw;
  const int seg = (f_hi - f_lo) * orig + taps;
  const int base = f_lo * orig - width;
  const float* xr = x + (size_t)b * ldx;
  for (int i = tid; i < seg; i += RS_TILE) {
    const int s = base + i;
    xs[i] = s >= 0 && s < len ? xr[s] : 0.0f;
  }
  __syncthreads();
  if (o >= ldo) return;
  float v = 0.0f;
  if (o < target) {
    const int f = o / nw, p = o - f * nw;
    const float* xp = xs + (f - f_lo) * orig;
    const float* kp = kt + p;
    double acc = 0.0;
#pragma unroll 4
    for (int t = 0; t < taps; ++t) acc = fma((double)xp[t], (double)kp[(size_t)t * nw], acc);
    v = (float)acc;
  }
  orow[o] = v;
}

}  // namespace

int resample_forward(const float* kt, int orig, int nw, int width, const float* x, int ldx, const int* lengths, int B, float* out, int ldo,
                     hipStream_t st) {
  IDX_CHECK(kt && x && out && lengths, "null pointer");
  IDX_CHECK(orig > 0 && nw > 0 && orig != nw && width > 0 && B > 0 && ldx >= 0 && ldo >= 0, "shape (equal rates need no resampling)");
  const int taps = 2 * width + orig;
  // the longest input segment a tile of outputs reads
  const long long seg = ((long long)(RS_TILE - 1) / nw + 1) * orig + taps;
  IDX_CHECK(seg * sizeof(float) <= 64 * 1024, "rate pair: a tile's input segment does not fit in LDS");
  for (int b = 0; b < B; ++b) {
    IDX_CHECK(lengths[b] >= 0 && lengths[b] <= ldx, "a row is longer than ldx");
    IDX_CHECK(((long long)nw * lengths[b] + orig - 1) / orig <= ldo, "ldo is shorter than a row's output");
    IDX_CHECK((long long)lengths[b] + taps + orig < (1ll << 31), "row too long");
  }
  if (ldo == 0) return 0;
  for (int b0 = 0; b0 < B; b0 += RS_ROWS) {
    const int nb = std::min(RS_ROWS, B - b0);
    RsRows r;
    for (int i = 0; i < RS_ROWS; ++i) r.len[i] = i < nb ? lengths[b0 + i] : 0;
    hipLaunchKernelGGL(resample_kernel, dim3(cdiv(ldo, RS_TILE), nb), dim3(RS_TILE), (size_t)seg * sizeof(float), st, out + (size_t)b0 * ldo,
                       x + (size_t)b0 * ldx, kt, r, ldx, ldo, orig, nw, width, taps);
    IDX_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace idxtts
