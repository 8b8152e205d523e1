// C wrapper around the reference's PLP and spectrogram feature code (runtime/kaldifeat/csrc), for tests/gen_plp_golden.py:
// the generator compiles this file with the reference's sources where they lie into a temporary directory, calls the two
// functions below and keeps only their outputs (tests/golden/plp_spectrogram.npz).  Nothing compiled is kept.
#include <cstdint>
#include <cstring>

#include "kaldifeat/csrc/feature-plp.h"
#include "kaldifeat/csrc/feature-spectrogram.h"

namespace {
void set_frame_opts(kaldifeat::FrameExtractionOptions *f, float sample_rate, float frame_length_ms, float frame_shift_ms, float preemph,
                    int remove_dc_offset, const char *window_type, int round_to_power_of_two, int snip_edges) {
  f->samp_freq = sample_rate;
  f->frame_length_ms = frame_length_ms;
  f->frame_shift_ms = frame_shift_ms;
  f->dither = 0.0f;
  f->preemph_coeff = preemph;
  f->remove_dc_offset = remove_dc_offset != 0;
  f->window_type = window_type;
  f->round_to_power_of_two = round_to_power_of_two != 0;
  f->snip_edges = snip_edges != 0;
}

int copy_out(const torch::Tensor &t, float *out, int cap_frames, int *dim_out) {
  torch::Tensor feats = t.contiguous();
  const int frames = (int)feats.size(0), dim = (int)feats.size(1);
  *dim_out = dim;
  if (frames > cap_frames) return -1;
  std::memcpy(out, feats.data_ptr<float>(), sizeof(float) * (size_t)frames * dim);
  return frames;
}
}  // namespace

extern "C" {

// wave: n samples (float, int16 value range); out: [frames][num_ceps] row-major, capacity cap_frames rows.
// Returns the number of frames, or -1 if out is too small.
int plp_ref_plp(const float *wave, int n, float sample_rate, float frame_length_ms, float frame_shift_ms, float preemph, int remove_dc_offset,
                const char *window_type, int round_to_power_of_two, int snip_edges, int num_bins, float low_freq, float high_freq,
                float vtln_warp, float vtln_low, float vtln_high, int lpc_order, int num_ceps, float compress_factor, int cepstral_lifter,
                float cepstral_scale, int use_energy, float energy_floor, int raw_energy, int htk_compat, float *out, int cap_frames,
                int *dim_out) {
  kaldifeat::PlpOptions opts;
  set_frame_opts(&opts.frame_opts, sample_rate, frame_length_ms, frame_shift_ms, preemph, remove_dc_offset, window_type,
                 round_to_power_of_two, snip_edges);
  opts.mel_opts.num_bins = num_bins;
  opts.mel_opts.low_freq = low_freq;
  opts.mel_opts.high_freq = high_freq;
  opts.mel_opts.vtln_low = vtln_low;
  opts.mel_opts.vtln_high = vtln_high;
  opts.lpc_order = lpc_order;
  opts.num_ceps = num_ceps;
  opts.compress_factor = compress_factor;
  opts.cepstral_lifter = cepstral_lifter;
  opts.cepstral_scale = cepstral_scale;
  opts.use_energy = use_energy != 0;
  opts.energy_floor = energy_floor;
  opts.raw_energy = raw_energy != 0;
  opts.htk_compat = htk_compat != 0;
  kaldifeat::Plp plp(opts);
  torch::Tensor w = torch::from_blob(const_cast<float *>(wave), {n}, torch::kFloat).clone();
  return copy_out(plp.ComputeFeatures(w, vtln_warp), out, cap_frames, dim_out);
}

// out: [frames][padded / 2 + 1]
int plp_ref_spectrogram(const float *wave, int n, float sample_rate, float frame_length_ms, float frame_shift_ms, float preemph,
                        int remove_dc_offset, const char *window_type, int round_to_power_of_two, int snip_edges, float energy_floor,
                        int raw_energy, float *out, int cap_frames, int *dim_out) {
  kaldifeat::SpectrogramOptions opts;
  set_frame_opts(&opts.frame_opts, sample_rate, frame_length_ms, frame_shift_ms, preemph, remove_dc_offset, window_type,
                 round_to_power_of_two, snip_edges);
  opts.energy_floor = energy_floor;
  opts.raw_energy = raw_energy != 0;
  kaldifeat::Spectrogram spec(opts);
  torch::Tensor w = torch::from_blob(const_cast<float *>(wave), {n}, torch::kFloat).clone();
  return copy_out(spec.ComputeFeatures(w, 1.0f), out, cap_frames, dim_out);
}

}  // extern "C"
