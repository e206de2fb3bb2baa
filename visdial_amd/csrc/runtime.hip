// Native step runtime: the model-level half of the C ABI (include/visdial_hip.h, "model-level entry points").
//
// The operator-level entry points replace single nn / rnn module calls; a host that composes them (Python,
// LuaJIT-FFI) must also own everything that makes the training step fast: stream fork/join, the skewed two-layer
// wavefront, the host-side length sort, workspace reuse, launch order.  This file puts that orchestration behind the
// ABI for every encoder / decoder plug-in pair of the reference (encoders/*.lua x decoders/{disc,gen}.lua) as the proxy
// object a Lua `model.lua` drives: vd_model_create ~ Model:__init (model.lua:10-63), vd_model_upload_batch ~ the batch
// re-layout + :cuda() copies (model.lua:255-294, dataloader.lua:410-475), vd_model_forward_backward ~
// Model:forwardBackward (model.lua:249-342), vd_model_update ~ clamp + adam + lr decay (model.lua:96-105),
// vd_model_retrieve / vd_model_ranks ~ Model:retrieveBatch + utils.computeRanks (model.lua:344-430, utils.lua:106-128).
// No arithmetic lives here: every tensor op is one of the operator-level launches of this same library.
//   rt_core.h      model object, helpers, nn.Linear / CatLinear / nn.SeqLSTM building blocks
//   rt_encoders.h  the 11 encoder plug-ins        rt_decoders.h  disc, gen + the forwardBackward / retrieve branches
//   rt_switches.h  the environment's switches of vd_model_create (host-only)
//
// Streams: main (option LSTM, criterion, decoder, optimiser), enc (encoder chains under a disc decoder), img (per-image
// projection + masks; also the history branch of lf-* / hre-*), tab (token sort + table gradient), copy (H2D uploads
// of the NEXT batch; two batch slots).
#include "rt_decoders.h"

using namespace vdrt;

vd_model::~vd_model() {}

namespace {

// [N x T] dataloader rows -> time-major [T x N] on the device; with `sorted` also the length-sort metadata of
// nn.py:SeqSort (stable sort by decreasing length, per-step active-row counts, gather indices)
//
// rollout_R > 0 (the history of a model created with VD_BEAM_ROLLOUT or VD_RETRIEVE_ROLLOUT, R rounds per dialog): rows n with n % R != 0 will be REWRITTEN on
// the device between the passes of a rollout (beam.hip R2), so their length is not known here.  They are laid out at full width,
// length T: by the paragraph below a row is skipped only BEFORE its claimed first token and masked per token inside its span, so a
// claim that covers leading zeros is exact and only costs work.  The sort then puts them in front of the caption rows (n % R == 0),
// which keep their true length; perm / inv / nact are fixed for every pass, and the pass writes tok and tok_sorted alike.
int upload_tokens(BatchSlot& sl, SeqTok& ss, const std::string& tag, const int32_t* rows_major, int N, int T, bool sorted, hipStream_t s,
                  int rollout_R = 0) {
  ss.T = T;
  ss.N = N;
  ss.present = true;
  ss.sorted = sorted;
  sl.wgrad_sig.clear();   // new lengths: the weight-gradient work list is rebuilt (rt_core.h wgrad_flush)
  const size_t TN = (size_t)T * N;
  // (+ up to 3 x T*N row-list entries; behind them, 16-byte aligned, the two segment tables of the live-row weight-gradient contractions)
  const size_t seg_at = (7 * TN + 2 * (size_t)N + T + 3) / 4 * 4, seg_ints = 4 * ((size_t)T + 1);
  const size_t total = sorted ? seg_at + 2 * seg_ints : TN;
  int32_t* stage = nullptr;
  VD_TRY(pin_get(sl.pinned, tag + ".stage", total * sizeof(int32_t), (void**)&stage));
  int32_t* tok = stage;
  std::vector<int> len(sorted ? N : 0);
  // A row's length is counted FROM ITS FIRST NON-ZERO TOKEN: the wavefront skips a row only at the steps before that token, where
  // maskZero() keeps the state at zero (exact), and applies the per-token mask inside the active span -- so a row that is not the
  // dataloader's right-aligned layout (left-aligned, interior zeros: reachable through the generic C ABI) is encoded exactly like the
  // masked per-step stack does.  For right-aligned rows this is the count of non-zero tokens.
  for (int n = 0; n < N; ++n) {
    int first = T;
    for (int t = 0; t < T; ++t) {
      const int32_t v = rows_major[(size_t)n * T + t];
      tok[(size_t)t * N + n] = v;
      if (v != 0 && first == T) first = t;
    }
    if (sorted) len[n] = rollout_R > 0 && n % rollout_R != 0 ? T : T - first;
  }
  if (sorted) {
    int32_t* tok_sorted = stage + TN;
    int32_t* fwd_idx = stage + 2 * TN;
    int32_t* inv_idx = stage + 3 * TN;
    int32_t* perm = stage + 4 * TN;
    int32_t* inv = perm + N;
    int32_t* nact = inv + N;
    std::vector<int> order(N);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });
    for (int i = 0; i < N; ++i) {
      perm[i] = order[i];
      inv[order[i]] = i;
    }
    ss.nact.assign(T, 0);
    for (int t = 0; t < T; ++t) {
      int c = 0;
      for (int n = 0; n < N; ++n) c += len[n] >= T - t;
      ss.nact[t] = c;
      nact[t] = c;
      for (int i = 0; i < N; ++i) {
        tok_sorted[(size_t)t * N + i] = tok[(size_t)t * N + perm[i]];
        fwd_idx[(size_t)t * N + i] = t * N + perm[i];
        inv_idx[(size_t)t * N + i] = t * N + inv[i];
      }
    }
    // non-pad (t, row) pairs of the sorted layout, in step order (rows [0, nact[t]) of step t)
    int32_t* act = nact + T;
    int na = 0;
    for (int t = 0; t < T; ++t)
      for (int i = 0; i < ss.nact[t]; ++i) act[na++] = t * N + i;
    const int n0 = T > 0 ? ss.nact[0] : 0;
    int32_t* prev1 = act + TN;
    for (int k = n0; k < na; ++k) prev1[k - n0] = act[k] - N;
    ss.n_act = na;
    ss.n_act1 = na - n0;
    for (int f = 0; f < 2; ++f) {   // wgrad_plan.h: t_first = 0 (dWx pairs), 1 (dWh pairs); a table holds at most T segments + the sentinel
      ss.seg_ksteps[f] = vdplan::live_segments(ss.nact.data(), T, N, f, &ss.seg_host[f]);
      memcpy(stage + seg_at + f * seg_ints, ss.seg_host[f].data(), ss.seg_host[f].size() * sizeof(vdplan::Seg));
    }
  }
  int32_t* dev = nullptr;
  VD_TRY(dev_get(sl.bufs, tag + ".dev", total * sizeof(int32_t), (void**)&dev));
  VD_HIP(hipMemcpyAsync(dev, stage, total * sizeof(int32_t), hipMemcpyHostToDevice, s));
  ss.tok = dev;
  if (sorted) {
    ss.tok_sorted = dev + TN;
    ss.fwd_idx = dev + 2 * TN;
    ss.inv_idx = dev + 3 * TN;
    ss.perm = dev + 4 * TN;
    ss.inv = ss.perm + N;
    ss.nact_dev = ss.inv + N;
    ss.act = ss.nact_dev + T;
    ss.act1 = ss.act + (T > 0 ? ss.nact[0] : 0);
    ss.prev1 = ss.act + TN;
    for (int f = 0; f < 2; ++f) ss.seg_dev[f] = dev + seg_at + f * seg_ints;
  }
  return VD_OK;
}

bool has(const std::string& s, const char* sub) { return s.find(sub) != std::string::npos; }

}  // namespace

// OptionCache (rt_core.h): resolve the NO candidate rows of a batch against the committed index and stage the rows it does not hold
int vdrt::option_cache_resolve(vd_model* m, BatchSlot& sl, const int32_t* options, long NO, int To, hipStream_t s) {
  OptionCache& oc = m->ocache;
  if (oc.index.T != To) {   // To is part of the key: the same tokens behind another number of trailing pads are another encoding
    oc.index.reset(To);
    ++oc.stamp;
  }
  const int32_t count = oc.index.size();
  RowIndex miss;
  miss.reset(To);
  int32_t* up = nullptr;
  VD_TRY(pin_get(sl.pinned, "opt.uid.stage", (size_t)NO * sizeof(int32_t), (void**)&up));
  for (long r = 0; r < NO; ++r) {
    const int32_t* row = options + (size_t)r * To;
    int32_t u = oc.index.find(row);
    if (u < 0) {
      int32_t l = miss.find(row);
      if (l < 0) l = miss.add(row);
      u = count + l;   // the table row the step fills for it
    }
    up[r] = u;
  }
  const int U = miss.size();
  sl.miss_keys.swap(miss.keys);
  sl.cached = true;
  sl.cache_stamp = oc.stamp;
  sl.opt_total = (int)NO;
  if (U > 0) {
    VD_TRY(upload_tokens(sl, sl.opt, "opt", sl.miss_keys.data(), U, To, false, s));
  } else {
    sl.opt.T = To;
    sl.opt.N = 0;
    sl.opt.present = true;
    sl.opt.sorted = false;
    sl.opt.tok = nullptr;
  }
  VD_TRY(dev_get(sl.bufs, "opt.uid", (size_t)NO * sizeof(int32_t), (void**)&sl.opt_uid));
  VD_HIP(hipMemcpyAsync(sl.opt_uid, up, (size_t)NO * sizeof(int32_t), hipMemcpyHostToDevice, s));
  sl.opt_sort_off = sl.opt_sort_perm = nullptr;   // no backward follows: the table gradient's token sort is not made
  return VD_OK;
}

// ---- prefix trees of a batch's candidates (VD_LHOOD_TREE; rt_core.h TreeChunk, rt_decoders.h Gen::retrieve_tree) --------------------
// option_in / option_out [N x O x T] host rows.  One tree per chunk of options [o0, o0 + C): level t holds one node per distinct
// (parent node, token) among the candidates still running at step t -- one open-addressing map per level keyed by (parent row, token);
// a parent row belongs to one round, so this is one map per (dialog, round) folded into one table.  Nodes are numbered in order of
// first occurrence inside their level (round-major), levels in step order.
struct TreeHost {
  int Tl = 0, Nw = 0;
  long n_nodes = 0;
  std::vector<int32_t> widths, enode, etgt;
  std::vector<std::vector<int32_t>> tok, par;   // per level
};

static void tree_build_range(const int32_t* oin, const int32_t* oout, int N, int O, int T, int o0, int C, TreeHost& th) {
  const long rows = (long)N * C;
  std::vector<int32_t> cur((size_t)rows);
  std::vector<uint8_t> alive((size_t)rows, 1);
  for (long r = 0; r < rows; ++r) cur[r] = (int32_t)(r / C);
  th = TreeHost();
  th.enode.assign((size_t)T * rows, 0);
  th.etgt.assign((size_t)T * rows, 0);
  std::vector<uint64_t> keys;
  std::vector<int32_t> vals;
  for (int t = 0; t < T; ++t) {
    long cnt = 0;
    for (long r = 0; r < rows; ++r) {
      if (alive[r] && oin[((size_t)(r / C) * O + o0 + r % C) * T + t] == 0) alive[r] = 0;
      cnt += alive[r];
    }
    if (cnt == 0) break;
    size_t cap = 16;
    while (cap < 2 * (size_t)cnt) cap <<= 1;
    keys.assign(cap, ~0ull);
    vals.assign(cap, -1);
    std::vector<int32_t> ltok, lpar;
    for (long r = 0; r < rows; ++r) {
      if (!alive[r]) continue;
      const size_t src = ((size_t)(r / C) * O + o0 + r % C) * T + t;
      const uint64_t key = ((uint64_t)(uint32_t)cur[r] << 32) | (uint32_t)oin[src];
      size_t pos = (size_t)((key * 0x9E3779B97F4A7C15ull) >> 20) & (cap - 1);
      while (keys[pos] != ~0ull && keys[pos] != key) pos = (pos + 1) & (cap - 1);
      if (keys[pos] == ~0ull) {
        keys[pos] = key;
        vals[pos] = (int32_t)ltok.size();
        ltok.push_back(oin[src]);
        lpar.push_back(cur[r]);
      }
      cur[r] = vals[pos];
      if (oout[src] != 0) {
        th.enode[(size_t)t * rows + r] = (int32_t)(th.n_nodes + cur[r]);
        th.etgt[(size_t)t * rows + r] = oout[src];
      }
    }
    th.widths.push_back((int32_t)ltok.size());
    th.n_nodes += (long)ltok.size();
    th.Nw = std::max<int>(th.Nw, (int)ltok.size());
    th.tok.push_back(std::move(ltok));
    th.par.push_back(std::move(lpar));
    th.Tl = t + 1;
  }
}

// the chunk's workspace by the nodes it actually holds: h and c of every level and layer (2H floats per node slot), the hoisted input
// projection of the layers above the first (4H), held to 4 GiB like the other heads' chunks; and the 32-bit byte offsets the kernels
// document -- the head's h rows (Tl * Nw * H * 4 bytes), one step's projection slice (Nw * 4H * 4 bytes), row indices below 2^31
static bool tree_chunk_fits(const TreeHost& th, long H, long layers) {
  const long slots = (long)th.Tl * th.Nw;
  return slots * (2 * H * layers + 4 * H * (layers - 1)) <= (1L << 30) && slots * H * 4 < (1L << 32) && (long)th.Nw * 4 * H * 4 < (1L << 32) &&
         slots < (1L << 31);
}

static int tree_chunks(vd_model* m, BatchSlot& sl, const int32_t* oin, const int32_t* oout, int N, int O, int T, int o0, int C, hipStream_t s) {
  TreeHost th;
  tree_build_range(oin, oout, N, O, T, o0, C, th);
  if (!tree_chunk_fits(th, m->p.rnnHiddenSize, m->p.numLayers) && C > 1) {   // does not fit: halve the option range
    VD_TRY(tree_chunks(m, sl, oin, oout, N, O, T, o0, C / 2, s));
    return tree_chunks(m, sl, oin, oout, N, O, T, o0 + C / 2, C - C / 2, s);
  }
  TreeChunk tc;
  tc.o0 = o0; tc.C = C; tc.Tl = th.Tl; tc.Nw = th.Nw; tc.n_nodes = th.n_nodes; tc.widths = th.widths;
  const size_t slots = (size_t)th.Tl * th.Nw, edges = (size_t)T * N * C;
  const size_t total = 2 * slots + (size_t)th.n_nodes + 2 * edges;
  const std::string tag = "tree." + std::to_string(sl.tree.size());
  int32_t *stage = nullptr, *dev = nullptr;
  VD_TRY(pin_get(sl.pinned, tag + ".stage", total * sizeof(int32_t), (void**)&stage));
  VD_TRY(dev_get(sl.bufs, tag, total * sizeof(int32_t), (void**)&dev));
  memset(stage, 0, 2 * slots * sizeof(int32_t));
  int32_t* nr = stage + 2 * slots;
  for (int t = 0; t < th.Tl; ++t) {
    const size_t w = th.tok[t].size();
    memcpy(stage + (size_t)t * th.Nw, th.tok[t].data(), w * sizeof(int32_t));
    memcpy(stage + slots + (size_t)t * th.Nw, th.par[t].data(), w * sizeof(int32_t));
    for (size_t n = 0; n < w; ++n) *nr++ = (int32_t)((size_t)t * th.Nw + n);
  }
  memcpy(nr, th.enode.data(), edges * sizeof(int32_t));
  memcpy(nr + edges, th.etgt.data(), edges * sizeof(int32_t));
  if (total) VD_HIP(hipMemcpyAsync(dev, stage, total * sizeof(int32_t), hipMemcpyHostToDevice, s));
  tc.mask2 = dev;
  tc.node_row = dev + 2 * slots;
  tc.enode = tc.node_row + th.n_nodes;
  tc.etgt = tc.enode + edges;
  sl.tree.push_back(std::move(tc));
  return VD_OK;
}

static int build_lhood_tree(vd_model* m, BatchSlot& sl, const int32_t* oin, const int32_t* oout, int N, int O, int T, hipStream_t s) {
  sl.tree.clear();
  sl.tree_ok = false;
  // an ill-formed batch -- a token behind a pad in any candidate (not one left-aligned run), or a token / target outside the vocabulary --
  // gets no tree: vd_model_retrieve_lhood then takes the length-ordered path, whose order kernels report the same condition
  const long V = m->p.vocabSize;
  for (size_t r = 0; r < (size_t)N * O; ++r) {
    bool run = true;
    for (int t = 0; t < T; ++t) {
      const int32_t a = oin[r * T + t], b = oout[r * T + t];
      if (a < 0 || a > V || b < 0 || b > V || (a != 0 && !run)) return VD_OK;
      run = run && a != 0;
    }
  }
  VD_TRY(tree_chunks(m, sl, oin, oout, N, O, T, 0, O, s));
  sl.tree_ok = true;
  return VD_OK;
}

extern "C" {

int vd_model_create(const vd_model_params* p, const char* encoder, const char* decoder, vd_model** out) {
  VD_CHECK_ARG(p && encoder && decoder && out, "vd_model_create: null argument");
  std::unique_ptr<Encoder> enc = make_encoder(encoder);
  std::unique_ptr<Decoder> dec = make_decoder(decoder);
  if (!enc || !dec) {
    vd_set_error("vd_model_create: unknown plug-in pair '%s' + '%s' (encoders: lf-ques, lf-ques-im, lf-ques-hist, lf-ques-im-hist, "
                 "lf-att-ques-im-hist, hre-ques-hist, hre-ques-im-hist, hrea-ques-im-hist, mn-ques-hist, mn-ques-im-hist, "
                 "mn-att-ques-im-hist; decoders: disc, gen)", encoder, decoder);
    return VD_ERR_ARG;
  }
  const std::string en(encoder);
  const bool use_im = has(en, "im"), is_att = has(en, "att") && !has(en, "hrea");
  VD_CHECK_ARG(p->rnnHiddenSize > 0 && p->rnnHiddenSize % 32 == 0 && p->embedSize > 0 && p->embedSize % 4 == 0 && p->vocabSize > 0 &&
                   p->maxQuesCount > 0 && p->numOptions > 0,
               "vd_model_create: rnnHiddenSize must be a positive multiple of 32, embedSize of 4; vocabSize, maxQuesCount, numOptions > 0");
  // the projection table [V+1 x 4H] of the option / decoder recurrences is gathered with 32-bit byte offsets (common.h)
  VD_CHECK_ARG(((long)p->vocabSize + 1) * 4 * p->rnnHiddenSize * 4 < (1L << 32),
               "vd_model_create: (vocabSize + 1) x 4 x rnnHiddenSize floats exceed 4 GB");
  VD_CHECK_ARG(!use_im || (p->imgFeatureSize > 0 && p->imgFeatureSize % 4 == 0), "vd_model_create: imgFeatureSize must be a positive multiple of 4");
  VD_CHECK_ARG(!is_att || (p->commonEmbeddingSize > 0 && p->commonEmbeddingSize % 4 == 0 && p->imgSpatialSize > 0),
               "vd_model_create: commonEmbeddingSize must be a positive multiple of 4 and imgSpatialSize > 0 for attention encoders");
  VD_CHECK_ARG(!(has(en, "hre") && use_im) || (p->imgEmbedSize > 0 && p->imgEmbedSize % 4 == 0),
               "vd_model_create: imgEmbedSize must be a positive multiple of 4 for hre*-ques-im-hist");
  VD_CHECK_ARG(p->dropout >= 0.f && p->dropout < 1.f, "vd_model_create: dropout must lie in [0, 1)");
  const int flags = vd_precision_flags(p->lstmBf16);
  VD_CHECK_ARG(flags >= 0, "vd_model_create: lstmBf16 must be 0, 1, 3, 6 or 9 (got %d)", p->lstmBf16);
  Switches sw;   // the environment's switches (rt_switches.h): a refused value touches no device and leaves no model behind
  VD_TRY(parse_switches(encoder, decoder, p->lstmBf16, &sw));
  VD_CHECK_ARG(sw.rollout_concat_end <= p->vocabSize, "vd_model_create: VD_ROLLOUT_CONCAT_END = %d is no token id: vocabSize is %d",
               sw.rollout_concat_end, (int)p->vocabSize);
  vd_model* m = new vd_model();
  m->p = *p;
  m->sw = sw;
  m->flags = flags;
  m->ocache.capacity = sw.option_cache_rows;
  if (m->p.numAttentionLayers < 1 || has(en, "lf-att")) m->p.numAttentionLayers = 1;   // (lf-att-ques-im-hist.lua:49 hard-codes one hop)
  if (m->p.numLayers < 1) m->p.numLayers = 2;        // opts.lua:27
  m->enc_name = encoder;
  m->dec_name = decoder;
  m->use_im = use_im;
  m->use_hist = has(en, "hist");
  m->is_att = is_att;
  m->is_graph = en.rfind("mn", 0) == 0 || en.rfind("lf-att", 0) == 0;
  m->lr = p->learningRate;
  m->streams = p->useStreams != 0;
  m->enc = std::move(enc);
  m->dec = std::move(dec);
  // wrapper = Sequential(encoder, decoder) -> getParameters (model.lua:45-55): embed | encoder tensors | decoder tensors
  m->spec.push_back(Tensor{"embed", 0, p->vocabSize + 1, p->embedSize, 0});
  m->enc->declare(m);
  m->dec->declare(m);
  long off = 0;
  for (size_t i = 0; i < m->spec.size(); ++i) {
    m->spec[i].off = off;
    m->index[m->spec[i].name] = (int)i;
    off += (m->spec[i].numel() + 3) / 4 * 4;  // every tensor 16-byte aligned (same layout as visdial_amd/params.py)
  }
  m->numel = off;
  auto fail = [&](int rc) {
    vd_model_destroy(m);
    return rc;
  };
  for (float** v : {&m->W, &m->G, &m->M, &m->V}) {
    if (hipMalloc((void**)v, off * sizeof(float)) != hipSuccess) {
      vd_set_error("vd_model_create: hipMalloc of %ld floats failed", off);
      return fail(VD_ERR_HIP);
    }
    (void)hipMemset(*v, 0, off * sizeof(float));
  }
  // Two lanes.  s_main (LEAST priority) carries the throughput work: option LSTM, criterion, optimiser.  s_side (GREATEST) carries
  // everything that runs beside it, in the host's enqueue order: the latency-bound encoder chains with their image prefetch / history
  // branch, the table-gradient chain and the batch uploads.  Their small workgroups take free slots ahead of the next big-kernel
  // workgroup.  The side work is ONE stream because its order is part of the schedule (profiles/r03_experiments.txt section 9): HIP gives
  // every priority class its own pool of GPU_MAX_HW_QUEUES hardware queues, and packets of one queue start in submission order.  As four
  // streams the side work ran in that order only where the four shared a queue (GPU_MAX_HW_QUEUES=1).  With a queue each, the side chains
  // ran beside each other as well as beside the main stream (in round 3 the HBM-bound table-gradient row sum beside the MFMA-bound dWh
  // contraction instead of behind the encoder backward), every option family took 5-7 % longer and the headline step 24.2 ms instead of
  // 22.3 (profiles/side_lane.txt).  One stream is one queue at any setting the host process chose.
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (hipStreamCreateWithPriority(&m->s_main, hipStreamNonBlocking, least) != hipSuccess) return fail(VD_ERR_HIP);
  if (hipStreamCreateWithPriority(&m->s_side, hipStreamNonBlocking, greatest) != hipSuccess) return fail(VD_ERR_HIP);
  // off-chain parameter-gradient work of a bf16 pass: middle priority = a queue of its own (rt_core.h, profiles/r03_experiments.txt section 21)
  if (least - greatest >= 2 &&
      hipStreamCreateWithPriority(&m->s_wg, hipStreamNonBlocking, (least + greatest) / 2) != hipSuccess)
    return fail(VD_ERR_HIP);
  m->ev_pool.resize(64);
  for (auto& e : m->ev_pool)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(VD_ERR_HIP);
  if (hipEventCreateWithFlags(&m->ev_loss, hipEventDisableTiming) != hipSuccess) return fail(VD_ERR_HIP);
  if (hipEventCreateWithFlags(&m->ev_enc_grads, hipEventDisableTiming) != hipSuccess) return fail(VD_ERR_HIP);
  if (hipEventCreateWithFlags(&m->ev_updated, hipEventDisableTiming) != hipSuccess) return fail(VD_ERR_HIP);
  for (auto& e : m->ev_prof)
    if (hipEventCreate(&e) != hipSuccess) return fail(VD_ERR_HIP);
  for (auto& sl : m->slot)
    if (hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) != hipSuccess)
      return fail(VD_ERR_HIP);
  *out = m;
  return VD_OK;
}

void vd_model_destroy(vd_model* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  for (float* v : {m->W, m->G, m->M, m->V})
    if (v) (void)hipFree(v);
  for (auto& kv : m->ws)
    if (kv.second.p) (void)hipFree(kv.second.p);
  for (auto& kv : m->ext_masks)
    if (kv.second.p) (void)hipFree(kv.second.p);
  if (m->ocache.table) (void)hipFree(m->ocache.table);
  for (auto& sl : m->slot) {
    for (auto& kv : sl.bufs)
      if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& kv : sl.pinned)
      if (kv.second.p) (void)hipHostFree(kv.second.p);
    if (sl.ready) (void)hipEventDestroy(sl.ready);
    if (sl.done) (void)hipEventDestroy(sl.done);
  }
  if (m->loss_host) (void)hipHostFree(m->loss_host);
  for (auto& e : m->ev_pool)
    if (e) (void)hipEventDestroy(e);
  if (m->ev_loss) (void)hipEventDestroy(m->ev_loss);
  if (m->ev_enc_grads) (void)hipEventDestroy(m->ev_enc_grads);
  if (m->ev_updated) (void)hipEventDestroy(m->ev_updated);
  for (auto& e : m->ev_prof)
    if (e) (void)hipEventDestroy(e);
  for (hipStream_t s : {m->s_main, m->s_side, m->s_wg})
    if (s) {
      (void)hipStreamDestroy(s);
    }
  delete m;
}

int64_t vd_model_num_tensors(const vd_model* m) { return m ? (int64_t)m->spec.size() : 0; }
int64_t vd_model_flat_size(const vd_model* m) { return m ? m->numel : 0; }

int vd_model_tensor_info(const vd_model* m, int64_t i, char* name64, int64_t* offset, int64_t* rows, int64_t* cols) {
  VD_CHECK_ARG(m && i >= 0 && i < (int64_t)m->spec.size(), "vd_model_tensor_info: bad index");
  const Tensor& t = m->spec[i];
  if (name64) {
    strncpy(name64, t.name.c_str(), 63);
    name64[63] = 0;
  }
  if (offset) *offset = t.off;
  if (rows) *rows = t.rows;
  if (cols) *cols = t.cols;
  return VD_OK;
}

int vd_model_flat_pointers(vd_model* m, float** W, float** dW, float** adam_m, float** adam_v) {
  VD_CHECK_ARG(m, "vd_model_flat_pointers: null model");
  m->ocache.flush();   // the host may write the weights through W
  if (W) *W = m->W;
  if (dW) *dW = m->G;
  if (adam_m) *adam_m = m->M;
  if (adam_v) *adam_v = m->V;
  return VD_OK;
}

void* vd_model_stream(vd_model* m) { return m ? (void*)m->s_main : nullptr; }

// Data-parallel gradient bucketing: the encoder's own tensors occupy the flat element range [lo, hi)
// (everything between the shared embedding and the decoder's tensors).  Under a `disc` decoder they are final when
// the encoder backward ends on the side lane, long before the option-LSTM backward does: a host makes its
// communication stream wait for that point and all-reduces the range underneath the rest of the step.
int vd_model_encoder_range(const vd_model* m, int64_t* lo, int64_t* hi) {
  VD_CHECK_ARG(m && lo && hi, "vd_model_encoder_range: null");
  const char* first_dec = m->dec_name == "disc" ? "opt.W" : "dec1.W";
  *lo = m->spec[1].off;
  *hi = m->spec[m->index.at(first_dec)].off;
  return VD_OK;
}
int vd_model_wait_encoder_grads(vd_model* m, void* stream) {
  VD_CHECK_ARG(m && m->enc_grads_recorded, "vd_model_wait_encoder_grads: no backward pass has been enqueued");
  VD_HIP(hipStreamWaitEvent((hipStream_t)stream, m->ev_enc_grads, 0));
  return VD_OK;
}

// Library-default initialisation (weight-init.lua is a no-op in the reference): SeqLSTM weight ~
// N(0, 1/sqrt(D+H)), bias 0 with the forget gate at 1; Linear weight and bias ~ U(+-1/sqrt(in)); LookupTable ~ N(0,1)
// with the pad row zero.
int vd_model_init_params(vd_model* m, uint64_t seed) {
  VD_CHECK_ARG(m, "vd_model_init_params: null model");
  std::mt19937_64 rng(seed);
  std::vector<float> host((size_t)m->numel, 0.f);
  const long H = m->p.rnnHiddenSize;
  for (const Tensor& t : m->spec) {
    float* w = host.data() + t.off;
    const long n = t.numel();
    if (t.kind == 0) {
      std::normal_distribution<float> nd(0.f, 1.f);
      for (long i = t.cols; i < n; ++i) w[i] = nd(rng);
    } else if (t.kind == 1) {
      std::normal_distribution<float> nd(0.f, 1.f / sqrtf((float)t.rows));
      for (long i = 0; i < n; ++i) w[i] = nd(rng);
    } else if (t.kind == 2) {
      for (long i = H; i < 2 * H; ++i) w[i] = 1.f;
    } else {
      const long in = t.kind == 3 ? t.cols : m->spec[m->index.at(t.name.substr(0, t.name.size() - 2) + ".W")].cols;
      const float s = 1.f / sqrtf((float)in);
      std::uniform_real_distribution<float> ud(-s, s);
      for (long i = 0; i < n; ++i) w[i] = ud(rng);
    }
  }
  VD_HIP(hipMemcpy(m->W, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  m->ocache.flush();
  return VD_OK;
}

// Batch attachments: names that start with '@' (no parameter's does).  "@dense_relevance" (loss.hip DT1): the relevance matrix [N x O] of the
// batch uploaded last, validated here, staged in pinned memory and copied on the upload lane behind the batch's own fields.  It waits for
// neither the main stream nor a running step, and leaves the answer-encoding cache alone: it touches no weight.
// "@dense_relevance_live" (`live`; loss.hip DL1 - DL5): the same matrix, validated with the same words under its own name; where some but not
// all rounds are live, the live rounds' option tokens are compacted and sorted behind the copy, so that the next training step runs the
// option recurrence and its gradients over those rows only.  An attachment replaces whatever was attached to the upload before.
static int attach_dense_relevance(vd_model* m, const float* host, int64_t n, bool live) {
  const char* who = live ? "vd_model_set_tensor: '@dense_relevance_live'" : "vd_model_set_tensor: '@dense_relevance'";
  VD_CHECK_ARG(!live || !(m->flags & VD_FLAG_BF16),
               "%s runs the live rounds' candidate rows through the fp32 / split option recurrence; this model was created with lstmBf16 = 1, "
               "whose compact-state recurrence is not covered: attach '@dense_relevance'", who);
  VD_CHECK_ARG(m->uploaded >= 0, "%s attaches to the batch uploaded last, and no batch has been uploaded", who);
  BatchSlot& sl = m->slot[m->uploaded];
  const int N = sl.q.N, O = m->p.numOptions;
  VD_CHECK_ARG(n == (int64_t)N * O, "%s holds N x O = %d x %d = %ld values for this batch, got %ld", who, N, O, (long)N * O, (long)n);
  double W = 0.0;
  std::vector<int32_t> live_idx, live_slot((size_t)N, -1);   // DL1
  for (int r = 0; r < N; ++r) {
    const float* row = host + (size_t)r * O;
    int minus = 0;
    double sum = 0.0;
    for (int o = 0; o < O; ++o) {
      const float v = row[o];
      VD_CHECK_ARG(v == -1.f || (v >= 0.f && v <= FLT_MAX),
                   "%s row %d, candidate %d = %g: a relevance is finite and >= 0, and a round without an annotation is a full row of -1", who, r,
                   o, (double)v);
      minus += v == -1.f;
      sum += v;
    }
    VD_CHECK_ARG(minus == 0 || minus == O, "%s row %d mixes -1 (%d entries) with relevances: a round without an annotation is a full row of -1",
                 who, r, minus);
    const double w = minus ? m->sw.dense_mix : sum > 0.0 ? 1.0 : 0.0;
    W += w;
    if (w > 0.0) {
      live_slot[r] = (int32_t)live_idx.size();
      live_idx.push_back(r);
    }
  }
  hipStream_t s = m->s_side;
  if (sl.used) VD_HIP(hipStreamWaitEvent(s, sl.done, 0));   // a step that reads an earlier attachment of this upload may still run
  if (sl.rel) VD_HIP(hipEventSynchronize(sl.ready));        // ... and its copy may still read the staging buffer
  float* stage = nullptr;
  VD_TRY(pin_get(sl.pinned, "rel.stage", (size_t)n * sizeof(float), (void**)&stage));
  memcpy(stage, host, (size_t)n * sizeof(float));
  VD_TRY(dev_get(sl.bufs, "rel", (size_t)n * sizeof(float), (void**)&sl.rel));
  VD_HIP(hipMemcpyAsync(sl.rel, stage, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
  sl.rel_W = W;
  sl.n_live = 0;
  const int n_live = (int)live_idx.size();
  // DL2: every round live (or none: W = 0 is refused at the step) is the all-rows attachment.  A slot resolved against the answer-encoding
  // cache holds the missing rows only and refuses a training step; a gen model holds no candidates to compact and refuses it too (DT5)
  if (live && n_live > 0 && n_live < N && sl.opt.present && !sl.cached && m->dec_name == "disc") {
    const int To = sl.opt.T;
    const long NL = (long)n_live * O, V1 = (long)m->p.vocabSize + 1;
    VD_CHECK_ARG((long)To * N * O <= 0x7fffffffL, "%s: %d x %d x %d option tokens do not fit the token sort's 32-bit row indices", who, To, N, O);
    int32_t *istage = nullptr, *idev = nullptr, *tok = nullptr, *work = nullptr;
    // (buffers sized by all N rounds: another live set on the same upload reallocates nothing)
    VD_TRY(pin_get(sl.pinned, "live.stage", (size_t)2 * N * sizeof(int32_t), (void**)&istage));
    memcpy(istage, live_slot.data(), (size_t)N * sizeof(int32_t));
    memcpy(istage + N, live_idx.data(), (size_t)n_live * sizeof(int32_t));
    VD_TRY(dev_get(sl.bufs, "live.idx", (size_t)2 * N * sizeof(int32_t), (void**)&idev));
    VD_HIP(hipMemcpyAsync(idev, istage, (size_t)(N + n_live) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    VD_TRY(dev_get(sl.bufs, "opt_live.dev", (size_t)To * N * O * sizeof(int32_t), (void**)&tok));
    VD_TRY(vd_dense_live_tokens_p(sl.opt.tok, sl.opt.N, To, sl.opt_uid, idev + N, n_live, O, tok, s));
    VD_TRY(dev_get(sl.bufs, "live.sort_off", (size_t)(V1 + 1) * sizeof(int32_t), (void**)&sl.live_sort_off));
    VD_TRY(dev_get(sl.bufs, "opt.sort_work", (size_t)2 * V1 * sizeof(int32_t), (void**)&work));   // the upload's sort is ahead on this lane
    VD_TRY(dev_get(sl.bufs, "live.sort_perm", (size_t)To * N * O * sizeof(int32_t), (void**)&sl.live_sort_perm));
    VD_TRY(vd_token_sort(tok, (long)To * NL, (int)V1, sl.live_sort_off, work, sl.live_sort_perm, s));
    sl.opt_live.T = To;
    sl.opt_live.N = (int)NL;
    sl.opt_live.present = true;
    sl.opt_live.sorted = false;
    sl.opt_live.tok = tok;
    sl.live_slot = idev;
    sl.n_live = n_live;
  }
  VD_HIP(hipEventRecord(sl.ready, s));   // the slot is ready when the attachment has landed too
  return VD_OK;
}

// "@img_regions" (attention.hip IR1 - IR6): the number of live regions of every image of the batch uploaded last, B counts that come as floats
// because that is the signature.  Validated here, staged in pinned memory as int32 and copied on the upload lane behind the batch's own
// fields, with attach_dense_relevance's waits: the image attention of every pass over this upload then walks the first cnt[b] regions of image
// b alone.  The hidden rows of the uploaded features stay the caller's: finite (IR5).  It touches no weight and no candidate, so the
// answer-encoding cache stays as it is.
static int attach_img_regions(vd_model* m, const float* host, int64_t n) {
  const char* who = "vd_model_set_tensor: '@img_regions'";
  VD_CHECK_ARG(m->uploaded >= 0, "%s attaches to the batch uploaded last, and no batch has been uploaded", who);
  VD_CHECK_ARG(m->is_att, "%s gives the image attention a region count per image, and encoder '%s' has no image attention (the encoders with it "
               "are mn-att-ques-im-hist and lf-att-ques-im-hist)", who, m->enc_name.c_str());
  BatchSlot& sl = m->slot[m->uploaded];
  const int S2 = m->p.imgSpatialSize * m->p.imgSpatialSize;
  VD_CHECK_ARG(n == (int64_t)sl.B, "%s holds one count per image, B = %d values for this batch, got %ld", who, sl.B, (long)n);
  for (int b = 0; b < sl.B; ++b) {
    const float v = host[b];
    VD_CHECK_ARG(v >= 1.f && v <= (float)S2 && v == (float)(int32_t)v,
                 "%s image %d = %g: a region count is an integer in 1 .. S2 = %d (imgSpatialSize^2)", who, b, (double)v, S2);
  }
  hipStream_t s = m->s_side;
  if (sl.used) VD_HIP(hipStreamWaitEvent(s, sl.done, 0));       // a step that reads an earlier attachment of this upload may still run
  if (sl.regions) VD_HIP(hipEventSynchronize(sl.ready));        // ... and its copy may still read the staging buffer
  int32_t* stage = nullptr;
  VD_TRY(pin_get(sl.pinned, "regions.stage", (size_t)n * sizeof(int32_t), (void**)&stage));
  for (int b = 0; b < sl.B; ++b) stage[b] = (int32_t)host[b];
  VD_TRY(dev_get(sl.bufs, "regions", (size_t)n * sizeof(int32_t), (void**)&sl.regions));
  VD_HIP(hipMemcpyAsync(sl.regions, stage, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  VD_HIP(hipEventRecord(sl.ready, s));   // the slot is ready when the attachment has landed too
  return VD_OK;
}

// "@ndcg" (loss.hip DT2): NDCG of every round of the current batch from the scores of its last forward / retrieval and its attached
// relevance matrix.  n = 2 N: the N doubles the kernel wrote, bit for bit, in the float buffer of the signature.
static int read_ndcg(vd_model* m, int which, float* host, int64_t n) {
  const char* who = "vd_model_get_tensor: '@ndcg'";
  if (!(m->cur >= 0 && m->scores)) return vd_set_error("%s ranks the scores of the last forward or retrieval, and there are none", who), VD_ERR_STATE;
  BatchSlot& b = m->slot[m->cur];
  if (!b.rel)
    return vd_set_error("%s needs the relevance matrix of the current batch: attach it with vd_model_set_tensor '@dense_relevance' after "
                        "the upload", who), VD_ERR_STATE;
  VD_CHECK_ARG(which == 0 && n == 2 * (int64_t)m->N, "%s returns N = %d doubles in 2 N = %d floats with selector 0, got n = %ld, selector %d", who,
               m->N, 2 * m->N, (long)n, which);
  double* out;
  VD_TRY(ws_get(m, "ndcg.rows", (size_t)m->N, &out));
  VD_HIP(hipStreamWaitEvent(m->s_main, b.ready, 0));   // an attachment made after the step began
  VD_TRY(vd_ndcg_p(m->scores, b.rel, out, m->N, m->O, m->s_main));
  VD_HIP(hipMemcpyAsync(host, out, (size_t)m->N * sizeof(double), hipMemcpyDeviceToHost, m->s_main));
  VD_HIP(hipEventRecord(b.done, m->s_main));
  VD_HIP(hipStreamSynchronize(m->s_main));
  return VD_OK;
}

int vd_model_set_tensor(vd_model* m, const char* name, const float* host, int64_t n) {
  if (m && name && host && name[0] == '@') {
    if (!strcmp(name, "@dense_relevance")) return attach_dense_relevance(m, host, n, false);
    if (!strcmp(name, "@dense_relevance_live")) return attach_dense_relevance(m, host, n, true);
    if (!strcmp(name, "@img_regions")) return attach_img_regions(m, host, n);
    VD_CHECK_ARG(false, "vd_model_set_tensor: unknown batch attachment '%s' (the library knows '@dense_relevance' and '@dense_relevance_live') "
                 "and, for the image attention, '@img_regions'", name);
  }
  VD_CHECK_ARG(m && name && host && m->index.count(name), "vd_model_set_tensor: unknown tensor '%s'", name ? name : "(null)");
  const Tensor& t = m->spec[m->index.at(name)];
  VD_CHECK_ARG(n == t.numel(), "vd_model_set_tensor: '%s' holds %ld values, got %ld", name, t.numel(), (long)n);
  VD_HIP(hipStreamSynchronize(m->s_main));
  VD_HIP(hipMemcpy(m->W + t.off, host, n * sizeof(float), hipMemcpyHostToDevice));
  m->ocache.flush();
  return VD_OK;
}

int vd_model_get_tensor(vd_model* m, const char* name, int which, float* host, int64_t n) {
  if (m && name && host && name[0] == '@') {
    if (!strcmp(name, "@ndcg")) return read_ndcg(m, which, host, n);
    VD_CHECK_ARG(false, "vd_model_get_tensor: unknown batch attachment '%s' (the library knows '@ndcg')", name);
  }
  VD_CHECK_ARG(m && name && host && m->index.count(name), "vd_model_get_tensor: unknown tensor '%s'", name ? name : "(null)");
  const Tensor& t = m->spec[m->index.at(name)];
  VD_CHECK_ARG(n == t.numel() && which >= 0 && which <= 3, "vd_model_get_tensor: bad size / selector");
  VD_HIP(hipStreamSynchronize(m->s_main));
  float* base[4] = {m->W, m->G, m->M, m->V};
  VD_HIP(hipMemcpy(host, base[which] + t.off, n * sizeof(float), hipMemcpyDeviceToHost));
  return VD_OK;
}

int vd_model_set_training(vd_model* m, int on) {
  VD_CHECK_ARG(m, "vd_model_set_training: null model");
  m->training = on != 0;
  if (on) m->ocache.flush();   // training steps move the weights (and a host that wrote them itself announces it this way)
  return VD_OK;
}

// pin the nn.Dropout noise of one call site (q_emb, h_emb, hatt, img_tr, iqc[, iqc2..], u; fuse; img); host == NULL
// clears all
int vd_model_set_dropout_mask(vd_model* m, const char* site, const uint8_t* host, int64_t n) {
  VD_CHECK_ARG(m, "vd_model_set_dropout_mask: null model");
  VD_HIP(hipStreamSynchronize(m->s_main));
  if (!host) {
    for (auto& kv : m->ext_masks)
      if (kv.second.p) VD_HIP(hipFree(kv.second.p));
    m->ext_masks.clear();
    return VD_OK;
  }
  VD_CHECK_ARG(site && n > 0, "vd_model_set_dropout_mask: bad arguments");
  void* p = nullptr;
  VD_TRY(dev_get(m->ext_masks, site, (size_t)n, &p));
  VD_HIP(hipMemcpy(p, host, (size_t)n, hipMemcpyHostToDevice));
  return VD_OK;
}

// Upload a batch in the dataloader's layout (dataloader.lua:324-339,378-475) into the free slot, asynchronously on the
// side lane: it may be called while the previous step is still executing.  Host buffers are consumed before return
// (staged into pinned memory), the device copy completes in the background.  Which fields are read follows the
// plug-in pair: hist / img_feat by the encoder name (opts.lua:54-67), options by `disc`, answer_in/out (training) and
// option_in/out (retrieval) by `gen`; fields the pair does not use may be NULL.
int vd_model_upload_batch(vd_model* m, const vd_batch* hb) {
  VD_CHECK_ARG(m && hb && hb->ques_fwd && hb->B > 0 && hb->Tq > 0, "vd_model_upload_batch: missing ques_fwd / B / Tq");
  VD_CHECK_ARG(!m->use_hist || (hb->hist && hb->Th > 0), "vd_model_upload_batch: encoder '%s' needs hist", m->enc_name.c_str());
  VD_CHECK_ARG(!m->use_im || hb->img_feat, "vd_model_upload_batch: encoder '%s' needs img_feat", m->enc_name.c_str());
  const bool disc = m->dec_name == "disc";
  VD_CHECK_ARG(!disc || (hb->options && hb->To > 0), "vd_model_upload_batch: decoder 'disc' needs options");
  // (decoder gen: answer_in/answer_out for training, option_in/option_out for retrieval, neither for generation)
  VdRange r("vd_model_upload_batch");
  BatchSlot& sl = m->slot[m->cur < 0 ? 0 : (m->cur ^ 1)];   // the slot the running step does not read
  // The side lane, behind whatever side work the host has enqueued for the running step: the prefetch of the pipelined loop follows that
  // step's table-gradient chain.  (Its place matters: profiles/r03_experiments.txt section 23b.)
  hipStream_t s = m->s_side;
  // the step that last read this slot may still be executing (the host runs ahead of the device): `done` is a main-stream event of an
  // EARLIER step call, so this wait holds up nothing on the lane that main is waiting for
  if (sl.used) VD_HIP(hipStreamWaitEvent(s, sl.done, 0));
  // ... and the previous upload INTO this slot may still be queued behind that wait, reading the slot's pinned staging
  // buffers: a host that runs two or more steps ahead without reading a loss (forward_backward loops, deferred loss)
  // would otherwise overwrite them under the copy.  In the pipelined training loop this returns at once.
  if (sl.uploaded) VD_HIP(hipEventSynchronize(sl.ready));
  sl.uploaded = true;
  sl.rel = nullptr;   // an attachment belongs to one upload
  sl.regions = nullptr;
  sl.rel_W = 0.0;
  sl.n_live = 0;
  sl.B = hb->B;
  const int R = m->p.maxQuesCount, N = hb->B * R, O = m->p.numOptions;
  const long NO = (long)N * O;
  for (SeqTok* t : {&sl.q, &sl.h, &sl.opt, &sl.ain, &sl.aout, &sl.oin, &sl.oout}) t->present = false;
  VD_TRY(upload_tokens(sl, sl.q, "q", hb->ques_fwd, N, hb->Tq, m->is_graph, s));
  // the history branch of the Sequential encoders runs as a length-sorted two-layer wavefront too (rt_encoders.h: HistoryBranch)
  const bool hist_wave = !m->is_graph && m->p.numLayers == 2;
  // VD_BEAM_ROLLOUT / VD_RETRIEVE_ROLLOUT: history rows >= 1 at full width (upload_tokens), and a history row has to hold a whole question
  // (beam.hip R2)
  const bool rollout = m->sw.beam_rollout || m->sw.retrieve_rollout;
  VD_CHECK_ARG(!(rollout && m->use_hist) || hb->Th >= hb->Tq,
               "vd_model_upload_batch: %s = 1 needs a history width Th = %d >= the question width Tq = %d",
               m->sw.beam_rollout ? "VD_BEAM_ROLLOUT" : "VD_RETRIEVE_ROLLOUT", hb->Th, hb->Tq);
  if (m->use_hist) VD_TRY(upload_tokens(sl, sl.h, "h", hb->hist, N, hb->Th, m->is_graph || hist_wave, s, rollout ? R : 0));
  if (m->use_im) {
    // [B x S*S x C] for the attention encoders (model.lua:262-265 keeps one map per image), [B x F] otherwise
    const size_t img_n = (size_t)hb->B * (m->is_att ? (size_t)m->p.imgSpatialSize * m->p.imgSpatialSize : 1) * m->p.imgFeatureSize;
    float* ip = nullptr;
    VD_TRY(pin_get(sl.pinned, "img.stage", img_n * sizeof(float), (void**)&ip));
    memcpy(ip, hb->img_feat, img_n * sizeof(float));
    VD_TRY(dev_get(sl.bufs, "img", img_n * sizeof(float), (void**)&sl.img));
    VD_HIP(hipMemcpyAsync(sl.img, ip, img_n * sizeof(float), hipMemcpyHostToDevice, s));
  }
  if (disc) {
    // Candidate answers repeat inside a batch on real VisDial (every round's 100 options draw from one answer pool: the
    // popular answers appear in most rounds), and the option encoding depends on the tokens alone (decoders/disc.lua:4-15):
    // encode each DISTINCT row once and address it through opt_uid (first-occurrence order; exact -- duplicates share
    // one forward value and their gradients add).  Synthetic batches have no repeats: the plain path, no extra kernels.
    sl.opt_uid = nullptr;
    sl.opt_total = (int)NO;
    sl.cached = false;
    const int To = hb->To;
    bool dedup = false;
    if (m->ocache.capacity > 0 && !m->training) {   // evaluation with the answer-encoding cache: only the rows it does not hold
      sl.opt_host.assign(hb->options, hb->options + (size_t)NO * To);
      VD_TRY(option_cache_resolve(m, sl, sl.opt_host.data(), NO, To, s));
    } else if (NO > 1) {
      std::vector<int32_t> uid((size_t)NO), uniq;
      uniq.reserve((size_t)NO * To);
      const size_t cap = (size_t)1 << (64 - __builtin_clzll((unsigned long long)(2 * NO)));   // power of two >= 2 NO
      std::vector<int32_t> table(cap, -1);
      int U = 0;
      for (long r = 0; r < NO; ++r) {
        const int32_t* row = hb->options + (size_t)r * To;
        uint64_t h = 1469598103934665603ull;
        for (int t = 0; t < To; ++t) h = (h ^ (uint32_t)row[t]) * 1099511628211ull;
        size_t pos = (size_t)(h ^ (h >> 29)) & (cap - 1);
        for (;;) {
          const int32_t u = table[pos];
          if (u < 0) {
            table[pos] = U;
            uid[r] = U++;
            uniq.insert(uniq.end(), row, row + To);
            break;
          }
          if (memcmp(uniq.data() + (size_t)u * To, row, (size_t)To * sizeof(int32_t)) == 0) {
            uid[r] = u;
            break;
          }
          pos = (pos + 1) & (cap - 1);
        }
      }
      if ((double)U <= 0.95 * (double)NO) {     // worth two extra [N*O x H] passes (gather / scatter-add)
        dedup = true;
        VD_TRY(upload_tokens(sl, sl.opt, "opt", uniq.data(), U, To, false, s));
        int32_t* up = nullptr;
        VD_TRY(pin_get(sl.pinned, "opt.uid.stage", (size_t)NO * sizeof(int32_t), (void**)&up));
        memcpy(up, uid.data(), (size_t)NO * sizeof(int32_t));
        VD_TRY(dev_get(sl.bufs, "opt.uid", (size_t)NO * sizeof(int32_t), (void**)&sl.opt_uid));
        VD_HIP(hipMemcpyAsync(sl.opt_uid, up, (size_t)NO * sizeof(int32_t), hipMemcpyHostToDevice, s));
      }
    }
    if (!dedup && !sl.cached) VD_TRY(upload_tokens(sl, sl.opt, "opt", hb->options, (int)NO, hb->To, false, s));   // [N x O x To] -> [To x N*O]
    sl.opt_sort_off = sl.opt_sort_perm = nullptr;
    if (!sl.cached) {   // counting sort of the option tokens behind the copies (the table gradient's row order depends on the batch alone)
      const long V1 = (long)m->p.vocabSize + 1, n = (long)sl.opt.T * sl.opt.N;
      int32_t* work;
      VD_TRY(dev_get(sl.bufs, "opt.sort_off", (size_t)(V1 + 1) * sizeof(int32_t), (void**)&sl.opt_sort_off));
      VD_TRY(dev_get(sl.bufs, "opt.sort_work", (size_t)2 * V1 * sizeof(int32_t), (void**)&work));
      VD_TRY(dev_get(sl.bufs, "opt.sort_perm", (size_t)n * sizeof(int32_t), (void**)&sl.opt_sort_perm));
      VD_TRY(vd_token_sort(sl.opt.tok, n, (int)V1, sl.opt_sort_off, work, sl.opt_sort_perm, s));
    }
  }
  if (!disc && hb->answer_in && hb->answer_out) {
    VD_TRY(upload_tokens(sl, sl.ain, "ain", hb->answer_in, N, hb->Ta, false, s));
    VD_TRY(upload_tokens(sl, sl.aout, "aout", hb->answer_out, N, hb->Ta, false, s));
  }
  sl.tree_ok = false;
  if (!disc && hb->option_in && hb->option_out) {                                               // model.lua:393-399
    VD_TRY(upload_tokens(sl, sl.oin, "oin", hb->option_in, (int)NO, hb->To, false, s));
    VD_TRY(upload_tokens(sl, sl.oout, "oout", hb->option_out, (int)NO, hb->To, false, s));
    if (m->sw.lhood_tree) VD_TRY(build_lhood_tree(m, sl, hb->option_in, hb->option_out, N, O, hb->To, s));
  }
  sl.has_gt = hb->answer_ind != nullptr;
  sl.gt_host.assign(N, 0);
  int32_t* gp = nullptr;
  VD_TRY(pin_get(sl.pinned, "gt.stage", (size_t)N * sizeof(int32_t), (void**)&gp));
  for (int n = 0; n < N; ++n) {
    const int g = hb->answer_ind ? hb->answer_ind[n] - 1 : 0;   // 1-based on disk (prepro.py:169)
    VD_CHECK_ARG(!hb->answer_ind || (g >= 0 && g < O), "vd_model_upload_batch: answer_ind[%d] = %d out of 1..%d", n, g + 1, O);
    sl.gt_host[n] = g;
    gp[n] = g;
  }
  VD_TRY(dev_get(sl.bufs, "gt", (size_t)N * sizeof(int32_t), (void**)&sl.gt));
  VD_HIP(hipMemcpyAsync(sl.gt, gp, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, s));
  VD_HIP(hipEventRecord(sl.ready, s));
  m->uploaded = (int)(&sl - m->slot);
  m->lhood_exec = -1;
  return VD_OK;
}

static int begin_step(vd_model* m, bool zero_grads, BatchSlot** out) {
  VD_CHECK_ARG(m && m->uploaded >= 0, "no batch uploaded");
  m->cur = m->uploaded;
  m->enc_grads_recorded = false;
  m->lhood_exec = -1;   // vd_model_option_rows describes the last step call (Gen::retrieve_begin sets it again)
  m->step_live = false;
  BatchSlot& b = m->slot[m->cur];
  m->N = b.q.N;
  m->O = m->p.numOptions;
  hipStream_t s = m->s_main;
  VD_HIP(hipStreamWaitEvent(s, b.ready, 0));
  if (zero_grads) VD_TRY(vd_memset(m->G, 0, m->numel * 4, s));                  // wrapper:zeroGradParameters (model.lua:68)
  VD_TRY(vd_memset(Wp(m, "embed"), 0, (long)m->p.embedSize * 4, s));            // LookupTableMaskZero zeroes the pad row
  b.used = true;
  *out = &b;
  return VD_OK;
}

// Model:forwardBackward on the uploaded batch (model.lua:249-342).  Enqueues only.
int vd_model_forward_backward(vd_model* m, int only_forward) {
  VdRange r(only_forward ? "vd_model_forward" : "vd_model_forward_backward");
  BatchSlot* b = nullptr;
  VD_TRY(begin_step(m, !only_forward, &b));
  if (!only_forward) m->ocache.flush();   // gradients are about to move the weights
  const int rc = m->dec->forward_backward(m, *b, only_forward != 0);
  VD_HIP(hipEventRecord(b->done, m->s_main));
  return rc;
}

// Model:retrieveBatch up to the option scores (model.lua:344-425): disc = option scores of a forward pass, gen = the
// log-likelihood of every candidate under the decoder.  Read them with vd_model_scores / vd_model_ranks.
int vd_model_retrieve(vd_model* m) {
  VdRange r("vd_model_retrieve");
  BatchSlot* b = nullptr;
  VD_TRY(begin_step(m, false, &b));
  const int rc = m->dec->retrieve(m, *b);
  VD_HIP(hipEventRecord(b->done, m->s_main));
  return rc;
}

// vd_model_retrieve for the generative decoder through the live-row log-likelihood head (csrc/lhood.hip)
int vd_model_retrieve_lhood(vd_model* m) {
  VdRange r("vd_model_retrieve_lhood");
  BatchSlot* b = nullptr;
  VD_TRY(begin_step(m, false, &b));
  const int rc = m->dec->retrieve_lhood(m, *b);
  VD_HIP(hipEventRecord(b->done, m->s_main));
  return rc;
}

// Model:generateAnswers, device side (model.lua:432-613).  vd_model_encode = `forwardBackward(batch, true, true)`
// (model.lua:464): encoder forward of the uploaded batch, state kept for vd_model_decode_begin.
int vd_model_encode(vd_model* m) {
  BatchSlot* b = nullptr;
  VD_TRY(begin_step(m, false, &b));
  m->gen_enc_out = nullptr;
  float* out = nullptr;
  const int rc = m->enc->forward(m, m->s_main, *b, &out);
  VD_HIP(hipEventRecord(b->done, m->s_main));
  if (rc == VD_OK) {
    m->gen_enc_out = out;
    m->gen_seq_len = m->enc->seqLen(*b);
  }
  return rc;
}
int vd_model_decode_begin(vd_model* m, const int32_t* rounds, int n) {
  VD_CHECK_ARG(m, "vd_model_decode_begin: null model");
  return m->dec->gen_begin(m, rounds, n);
}
int vd_model_decode_step(vd_model* m, const int32_t* tokens, float* host_logprobs) {
  VD_CHECK_ARG(m, "vd_model_decode_step: null model");
  return m->dec->gen_step(m, tokens, host_logprobs);
}
int vd_model_decode_select(vd_model* m, const int32_t* src, int n_keep) {
  VD_CHECK_ARG(m, "vd_model_decode_select: null model");
  return m->dec->gen_select(m, src, n_keep);
}
int vd_model_beam_search(vd_model* m, int beam_size, int beam_len, int start_token, int end_token, int32_t* host_tokens,
                         double* host_scores) {
  VD_CHECK_ARG(m, "vd_model_beam_search: null model");
  VdRange r("vd_model_beam_search");
  return m->dec->gen_beam_search(m, beam_size, beam_len, start_token, end_token, host_tokens, host_scores);
}
int vd_model_sample(vd_model* m, int beam_len, int start_token, int end_token, double temperature, const double* host_uniforms,
                    int32_t* host_tokens, double* host_loglik) {
  VD_CHECK_ARG(m, "vd_model_sample: null model");
  VdRange r("vd_model_sample");
  return m->dec->gen_sample(m, beam_len, start_token, end_token, temperature, host_uniforms, host_tokens, host_loglik);
}

// waits for the loss of the last vd_model_forward_backward: disc = mean cross-entropy over the rounds, gen = summed
// NLL over the non-pad answer tokens (SequencerCriterion of ClassNLLCriterion, model.lua:32-36)
int vd_model_loss(vd_model* m, float* loss) {
  VD_CHECK_ARG(m && loss && m->cur >= 0 && m->loss_n > 0, "vd_model_loss: nothing to read");
  VD_HIP(hipEventSynchronize(m->ev_loss));
  double s = 0;
  for (long i = 0; i < m->loss_n; ++i) s += m->loss_host[i];
  *loss = (float)(m->loss_is_sum ? s : s / (m->loss_div > 0.0 ? m->loss_div : (double)m->loss_n));
  return VD_OK;
}

// [gradient already reduced by the caller] -> clamp(-5, 5) -> adam -> lr decay (model.lua:96-105; optim_updates.lua:62-91)
int vd_model_update(vd_model* m, float gscale) {
  VD_CHECK_ARG(m, "vd_model_update: null model");
  VdRange r("vd_model_update: clamp + adam");
  m->adam_t += 1;
  m->ocache.flush();
  const double t = m->adam_t;
  const float step = (float)(m->lr * sqrt(1.0 - pow(0.999, t)) / (1.0 - pow(0.9, t)));
  const float clip_norm = (float)m->sw.grad_clip_norm, decay = (float)(m->lr * m->sw.weight_decay);   // lr before this step's decay (WD1)
  if (clip_norm > 0.f || decay > 0.f) {   // decided on the fp32 values the kernels see: a lambda whose lr * lambda rounds to 0 is off
    // VD_GRAD_CLIP_NORM / VD_WEIGHT_DECAY (elementwise.hip GC1-GC3, WD1): the norm of gscale * G and its scale stay on the device
    float* work = nullptr;
    if (clip_norm > 0.f) {
      VD_TRY(ws_get(m, "upd.clip_work", (size_t)vd_clip_work_floats(), &work));
      VD_TRY(vd_grad_clip_scale_p(m->G, m->numel, gscale, clip_norm, work, m->s_main));
    }
    VD_TRY(vd_clip_decay_adam_p(m->W, m->G, m->M, m->V, m->numel, gscale, 5.0f, 0.9f, 0.999f, 1e-8f, step, work, decay, m->s_main));
  } else {
    VD_TRY(vd_clamp_adam(m->W, m->G, m->M, m->V, m->numel, gscale, 5.0f, 0.9f, 0.999f, 1e-8f, step, m->s_main));
  }
  VD_HIP(hipEventRecord(m->ev_updated, m->s_main));
  m->updated_recorded = true;
  if (m->lr > m->p.minLRate) m->lr *= m->p.lrDecayRate;
  m->step += 1;
  return VD_OK;
}

int vd_model_learning_rate(vd_model* m, double* lr, int set) {
  VD_CHECK_ARG(m && lr, "vd_model_learning_rate: null");
  if (set) m->lr = *lr;
  else *lr = m->lr;
  return VD_OK;
}

// scores [N x O] of the last forward / retrieval (host buffer)
int vd_model_scores(vd_model* m, float* host, int64_t n) {
  VD_CHECK_ARG(m && host && m->cur >= 0 && m->scores && n == (int64_t)m->N * m->O, "vd_model_scores: no scores / bad size");
  VD_HIP(hipStreamSynchronize(m->s_main));
  VD_HIP(hipMemcpy(host, m->scores, n * sizeof(float), hipMemcpyDeviceToHost));
  return VD_OK;
}

// utils.computeRanks on the scores of the last forward / retrieval: use_gt -> ranks_out[N] (rank of the ground-truth
// option), else ranks_out[N x O] (rank of every option), 1-based (utils.lua:106-128)
int vd_model_ranks(vd_model* m, int use_gt, int32_t* ranks_out) {
  VD_CHECK_ARG(m && ranks_out && m->cur >= 0 && m->scores, "vd_model_ranks: nothing to rank");
  const int N = m->N, O = m->O;
  const BatchSlot& b = m->slot[m->cur];
  VD_CHECK_ARG(!use_gt || b.has_gt, "vd_model_ranks: the batch carries no answer_ind");
  int32_t* ranks;
  VD_TRY(ws_get(m, "opt.ranks", (size_t)N * O, &ranks));
  VD_TRY(vd_ranks(m->scores, ranks, N, O, m->s_main));
  std::vector<int32_t> host((size_t)N * O);
  VD_HIP(hipMemcpyAsync(host.data(), ranks, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, m->s_main));
  VD_HIP(hipStreamSynchronize(m->s_main));
  if (use_gt) {
    for (int n = 0; n < N; ++n) ranks_out[n] = host[(size_t)n * O + b.gt_host[n]];
  } else {
    memcpy(ranks_out, host.data(), host.size() * sizeof(int32_t));
  }
  return VD_OK;
}

// device time of three kernel families inside the last training step, ms.  `disc` pairs: the option LSTM [fwd, bwd, dWh];
// `gen` pairs over a Sequential encoder with a history branch: [history branch fwd, history branch bwd, vocabulary projection +
// criterion + their gradients]; zeros when the last call was not such a step
int vd_model_family_ms(vd_model* m, float* ms3) {
  VD_CHECK_ARG(m && ms3, "vd_model_family_ms: null");
  ms3[0] = ms3[1] = ms3[2] = 0.f;
  if (!m->prof_valid) return VD_OK;
  VD_HIP(hipStreamSynchronize(m->s_main));
  VD_HIP(hipEventElapsedTime(&ms3[0], m->ev_prof[0], m->ev_prof[1]));
  VD_HIP(hipEventElapsedTime(&ms3[1], m->ev_prof[2], m->ev_prof[3]));
  VD_HIP(hipEventElapsedTime(&ms3[2], m->ev_prof[4], m->ev_prof[5]));
#ifdef VD_PROBE_PHASES
  { float t[12]; hipEvent_t* pe = vdrt::probe_events();
    for (int i = 1; i < 6; ++i) (void)hipEventElapsedTime(&t[i], m->ev_prof[0], m->ev_prof[i]);
    for (int i = 0; i < 5; ++i) (void)hipEventElapsedTime(&t[6 + i], m->ev_prof[0], pe[i]);
    fprintf(stderr, "PHASES (ms after option-fwd start) main: fwd end %.2f | bwd %.2f -> %.2f | dWh %.2f -> %.2f | all joined %.2f  ||  enc fwd end %.2f | enc bwd chain end %.2f | "
            "wg chain end %.2f | table chain end %.2f\n", t[1], t[2], t[3], t[4], t[5], t[10], t[6], t[7], t[8], t[9]); }
#endif
  return VD_OK;
}

// rows the option LSTM executed for the batch of the LAST STEP (vd_model_forward_backward / vd_model_retrieve) vs the N * O candidates
// they stand for (decoder disc); before any step: of the uploaded batch.  In a pipelined loop that is NOT the prefetched batch.
// After a training step on "@dense_relevance_live" with some but not all rounds live: (n_live * O, N * O).
// After vd_model_retrieve_lhood (decoder gen): the (step, candidate) rows that lay in a row group the candidate recurrence ran, summed
// over the chunks, vs To * N * O; any other step call or upload afterwards brings the answer above back.
int vd_model_option_rows(vd_model* m, int64_t* executed, int64_t* total) {
  VD_CHECK_ARG(m && executed && total && (m->cur >= 0 || m->uploaded >= 0), "vd_model_option_rows: no batch uploaded");
  if (m->lhood_exec >= 0) {   // the last step call was vd_model_retrieve_lhood (decoder gen)
    *executed = m->lhood_exec;
    *total = m->lhood_total;
    return VD_OK;
  }
  const BatchSlot& b = m->slot[m->cur >= 0 ? m->cur : m->uploaded];
  *executed = b.opt.present ? (m->step_live ? b.opt_live.N : b.opt.N) : 0;   // (a live dense step: the live rounds' rows, loss.hip DL3)
  *total = b.opt.present ? (b.opt_total ? b.opt_total : b.opt.N) : 0;
  return VD_OK;
}

int vd_model_synchronize(vd_model* m) {
  VD_CHECK_ARG(m, "vd_model_synchronize: null model");
  for (hipStream_t s : {m->s_side, m->s_wg, m->s_main})
    if (s) VD_HIP(hipStreamSynchronize(s));
  return VD_OK;
}

}  // extern "C"
