// Native step runtime: the switches vd_model_create reads from the environment (include/visdial_hip.h documents each at the call it changes;
// how to add one).  Host-only -- the C library and <string>, no HIP header, no common.h -- so that a stand-alone program with
// its own vd_set_error can run the parser under a host sanitizer.  Included by rt_core.h.
//
// What is accepted, written down once (hosts and tests match on the refusal sentences):
//  - VD_OPTION_CACHE goes through atol, so text is tolerated; <= 0 is off, 1 is VD_OPTION_CACHE_DEFAULT_ROWS, larger is the capacity in rows,
//    >= 2^30 is refused.  VD_LHOOD_TREE is atol(e) > 0.  The two are older than the strict readers.
//  - integer switches refuse an empty string, trailing characters, ERANGE and values above INT32_MAX.
//  - real switches refuse an empty string and trailing characters, and a NaN fails both comparisons of its range: VD_SAMPLE_TOPP in (0, 1],
//    VD_BEAM_DIVERSITY in [0, FLT_MAX] (lambda is applied in fp32), VD_BEAM_LENGTH_PENALTY in [0, DBL_MAX].  errno is not looked at.
//  - the sampling and beam variables and VD_BEAM_ROLLOUT are not read for decoder disc, VD_RETRIEVE_ROLLOUT not for decoder gen: garbage in
//    them is ignored there.  VD_ROLLOUT_ENCODER and VD_ROLLOUT_CONCAT_END are validated for every model.
//  - the training knobs are read for both decoders: VD_LABEL_SMOOTHING in [0, 1), VD_GRAD_CLIP_NORM and VD_WEIGHT_DECAY in [0, FLT_MAX]
//    (both are applied in fp32); 0 or unset = off.  VD_DENSE_MIX in [0, 1], for both decoders too.
#pragma once
#include <errno.h>
#include <float.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>

void vd_set_error(const char* fmt, ...);

namespace vdrt {

static constexpr long VD_OPTION_CACHE_DEFAULT_ROWS = 262144;   // 512 MiB of fp32 state at H = 512

struct Switches {                     // (decoder the variable is read for) what the call it belongs to does with it
  long option_cache_rows = 0;         // VD_OPTION_CACHE (disc): capacity of the answer-encoding cache; 0 = off
  bool lhood_tree = false;            // VD_LHOOD_TREE (gen): vd_model_retrieve_lhood scores over a prefix tree of the candidates
  int sample_topk = 0;                // VD_SAMPLE_TOPK, VD_SAMPLE_TOPP (gen): vd_model_sample draws from the top-k / nucleus kept set; 0 / 1 = off
  double sample_topp = 1.0;
  int beam_groups = 1;                // VD_BEAM_GROUPS, VD_BEAM_DIVERSITY (gen): vd_model_beam_search searches in that many groups per round with
  double beam_diversity = 0.5;        // that Hamming diversity and returns every group's answer; 1 = the plain search
  int beam_min_len = 0, beam_no_repeat = 0;   // VD_BEAM_MIN_LEN, VD_BEAM_NO_REPEAT, VD_BEAM_LENGTH_PENALTY (gen): the constraints of the search
  double beam_length_penalty = 0.0;           // (beam.hip C1-C6); 0 = off
  // VD_BEAM_ROLLOUT (gen), VD_RETRIEVE_ROLLOUT (disc): the search / vd_model_retrieve answer round r on a history of the model's own answers /
  // picks (beam.hip R1-R6 / E1-E5); an upload then lays out history rows >= 1 at full width (runtime.hip upload_tokens)
  bool beam_rollout = false, retrieve_rollout = false;
  bool rollout_round = false;         // VD_ROLLOUT_ENCODER = round: a rollout's passes >= 1 encode one round alone (Encoder::forward_round)
  // VD_ROLLOUT_CONCAT_END (both): the <END> id; a rollout then writes CONCATENATED history rows (beam.hip CH1-CH6: row r + 1 = row r, <END>, the
  // question, the answer) instead of per-round rows; 0 = off.  vd_model_create refuses a value above vocabSize (it knows V; this header does not)
  int rollout_concat_end = 0;
  // the training knobs (both): vd_model_forward_backward(m, 0) trains on targets smoothed by label_smoothing (loss.hip LS1-LS4);
  // vd_model_update clips the flat gradient to the global norm grad_clip_norm and decays the weights by weight_decay (elementwise.hip
  // GC1-GC3, WD1); 0 = off
  double label_smoothing = 0.0;       // VD_LABEL_SMOOTHING
  double grad_clip_norm = 0.0;        // VD_GRAD_CLIP_NORM
  double weight_decay = 0.0;          // VD_WEIGHT_DECAY
  // VD_DENSE_MIX (both): the weight mu of a round that is not annotated in a training step on a batch that carries "@dense_relevance"
  // (loss.hip DT3); 0 = such rounds do not train
  double dense_mix = 0.0;
};

// The typed readers.  An unset variable leaves *out alone; a refusal is "vd_model_create: NAME = 'text' <must>".
inline bool switch_refused(const char* name, const char* e, const char* must) {
  vd_set_error("vd_model_create: %s = '%s' %s", name, e, must);
  return false;
}
inline bool read_int(const char* name, long lo, const char* must, int* out) {
  const char* e = getenv(name);
  if (!e) return true;
  char* end = nullptr;
  errno = 0;
  const long v = strtol(e, &end, 10);
  if (!(*e && end && !*end && errno == 0 && v >= lo && v <= INT32_MAX)) return switch_refused(name, e, must);
  *out = (int)v;
  return true;
}
inline bool read_real(const char* name, double lo, bool lo_open, double hi, const char* must, double* out) {
  const char* e = getenv(name);
  if (!e) return true;
  char* end = nullptr;
  const double v = strtod(e, &end);
  if (!(*e && end && !*end && (lo_open ? v > lo : v >= lo) && v <= hi)) return switch_refused(name, e, must);
  *out = v;
  return true;
}
inline bool read_choice(const char* name, const char* off, const char* on, const char* must, bool* out) {   // 0 / 1 and full / round
  const char* e = getenv(name);
  if (!e) return true;
  if (strcmp(e, off) && strcmp(e, on)) return switch_refused(name, e, must);
  *out = !strcmp(e, on);
  return true;
}

// 0 (VD_OK), or -1 (VD_ERR_ARG) after vd_set_error; touches no device.  The checks keep the order the switches were added in -- a cross-check
// sits behind the last reader it depends on -- which is the order two bad values are reported in.
inline int parse_switches(const char* encoder, const char* decoder, int lstmBf16, Switches* out) {
#define VD_SWITCH_NEEDS(cond, ...) \
  if (!(cond)) return vd_set_error(__VA_ARGS__), -1
  const bool gen = std::string(decoder) == "gen", disc = std::string(decoder) == "disc";
  const char *int0 = "must be an integer >= 0 (0 = off)", *flag = "must be 1 or 0 (0 = off)";
  Switches sw;
  if (const char* e = getenv("VD_OPTION_CACHE")) {
    const long v = atol(e);
    sw.option_cache_rows = v <= 0 ? 0 : v == 1 ? VD_OPTION_CACHE_DEFAULT_ROWS : v;
  }
  VD_SWITCH_NEEDS(!sw.option_cache_rows || disc,
                  "vd_model_create: VD_OPTION_CACHE caches the candidate encodings of decoder 'disc'; this model's decoder is '%s'", decoder);
  VD_SWITCH_NEEDS(!sw.option_cache_rows || lstmBf16 != 1,
                  "vd_model_create: VD_OPTION_CACHE needs the state-only option recurrence, which the compact bf16 recurrence (lstmBf16 = 1) "
                  "does not have");
  VD_SWITCH_NEEDS(sw.option_cache_rows < (1L << 30), "vd_model_create: VD_OPTION_CACHE = %ld rows is out of range", sw.option_cache_rows);
  if (const char* e = getenv("VD_LHOOD_TREE")) sw.lhood_tree = atol(e) > 0;
  VD_SWITCH_NEEDS(!sw.lhood_tree || gen,
                  "vd_model_create: VD_LHOOD_TREE scores the candidates of decoder 'gen' over a prefix tree; this model's decoder is '%s'", decoder);
  VD_SWITCH_NEEDS(!sw.lhood_tree || lstmBf16 != 1,
                  "vd_model_create: VD_LHOOD_TREE runs the exact fp32 tree recurrence (VD_FLAG_TREE), which the compact bf16 recurrence "
                  "(lstmBf16 = 1) does not have");
  if (gen && !(read_int("VD_SAMPLE_TOPK", 0, int0, &sw.sample_topk) &&
               read_real("VD_SAMPLE_TOPP", 0.0, true, 1.0, "must be a real in (0, 1] (1 = off)", &sw.sample_topp) &&
               read_int("VD_BEAM_GROUPS", 1, "must be an integer >= 1 (1 = off)", &sw.beam_groups) &&
               read_real("VD_BEAM_DIVERSITY", 0.0, false, (double)FLT_MAX, "must be a finite real >= 0", &sw.beam_diversity) &&
               read_int("VD_BEAM_MIN_LEN", 0, int0, &sw.beam_min_len) && read_int("VD_BEAM_NO_REPEAT", 0, int0, &sw.beam_no_repeat) &&
               read_real("VD_BEAM_LENGTH_PENALTY", 0.0, false, DBL_MAX, "must be a finite real >= 0 (0 = off)", &sw.beam_length_penalty) &&
               read_choice("VD_BEAM_ROLLOUT", "0", "1", flag, &sw.beam_rollout)))
    return -1;
  VD_SWITCH_NEEDS(!sw.beam_rollout || sw.beam_groups == 1,
                  "vd_model_create: VD_BEAM_ROLLOUT = 1 with VD_BEAM_GROUPS = %d: a rollout feeds ONE answer per round back, and the choice "
                  "among a round's groups is the host's", sw.beam_groups);
  if (disc && !read_choice("VD_RETRIEVE_ROLLOUT", "0", "1", flag, &sw.retrieve_rollout)) return -1;
  VD_SWITCH_NEEDS(!sw.retrieve_rollout || sw.option_cache_rows == 0,
                  "vd_model_create: VD_RETRIEVE_ROLLOUT = 1 with VD_OPTION_CACHE: a cached batch carries only the candidate rows the cache did "
                  "not hold, and the rollout reads a picked candidate's tokens from the batch; combining the two is left for a follow-up");
#undef VD_SWITCH_NEEDS
  bool round = false;
  if (!read_choice("VD_ROLLOUT_ENCODER", "full", "round", "must be 'full' or 'round' (unset = full)", &round)) return -1;
  // `round` is kept only where a rollout applies: without one, or with an encoder without a history, both calls run the plain search / retrieval
  sw.rollout_round = round && (sw.beam_rollout || sw.retrieve_rollout) && strstr(encoder, "hist");
  if (!read_int("VD_ROLLOUT_CONCAT_END", 0, "must be an integer >= 0: the <END> token id (0 = off)", &sw.rollout_concat_end)) return -1;
  // kept, like `round`, only where a rollout applies; there it is for the encoders that read the running concatenation.  With `round` the later
  // passes continue the history stack from a carried state over the new tokens alone (rt_encoders.h history_round_concat)
  if (!((sw.beam_rollout || sw.retrieve_rollout) && strstr(encoder, "hist"))) sw.rollout_concat_end = 0;
  if (sw.rollout_concat_end && strncmp(encoder, "lf-", 3))
    return vd_set_error("vd_model_create: VD_ROLLOUT_CONCAT_END = %d with encoder '%s': its history is one row per round (beam.hip R2 / E4), not "
                        "the running concatenation of the dialog; the concatenation rule (CH1-CH6) is for lf-ques-hist, lf-ques-im-hist and "
                        "lf-att-ques-im-hist", sw.rollout_concat_end, encoder), -1;
  // all three are applied in fp32: the largest float below 1 closes [0, 1)
  const char* real0 = "must be a finite real >= 0 (0 = off)";
  if (!(read_real("VD_LABEL_SMOOTHING", 0.0, false, 1.0 - (double)FLT_EPSILON / 2, "must be a real in [0, 1) (0 = off)", &sw.label_smoothing) &&
        read_real("VD_GRAD_CLIP_NORM", 0.0, false, (double)FLT_MAX, real0, &sw.grad_clip_norm) &&
        read_real("VD_WEIGHT_DECAY", 0.0, false, (double)FLT_MAX, real0, &sw.weight_decay)))
    return -1;
  if (!read_real("VD_DENSE_MIX", 0.0, false, 1.0, "must be a finite real in [0, 1] (0 = rounds without an annotation do not train)",
                 &sw.dense_mix))
    return -1;
  *out = sw;
  return 0;
}

}  // namespace vdrt
