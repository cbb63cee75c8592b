// Host side of libttx_hip.so: the C ABI of include/ttx.h, the runtime around the kernels (sessions, workspaces, hipGraphs,
// polling loops under drive_sessions, slot pools) and the loop / bookkeeping kernels (ttx_loop_kernels.hip.h).  The GEMM and attention families
// live in ttx_gemm.hip / ttx_attn.hip and are reached through the launchers of ttx_internal.h.
// No CPU fallback exists anywhere in this library: without a gfx950 device every entry point fails.
#include "ttx_internal.h"
#include "ttx_admit.h"
#include "ttx_drive.h"
#include "ttx_loop_kernels.hip.h"
#include "ttx_metrics.hip.h"
#include "ttx_score.hip.h"
#include "ttx_score_list.hip.h"
#include "ttx_fold.hip.h"
#include "ttx_alternatives.hip.h"
#include "ttx_attn_probs.hip.h"
#include "ttx_sample.hip.h"
#include "ttx_logit_bias.hip.h"
#include "ttx_syntax.hip.h"
#include "ttx_logq.hip.h"
#include "ttx_sbs.hip.h"
#include "ttx_sbs_pool.hip.h"
#include "ttx_beam_mask.hip.h"
#include "ttx_proposal.hip.h"
#include "ttx_tokenizer.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

using namespace ttx;

// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int ttx::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

static void layout_add(ttx_model* m, const std::string& name, size_t numel, size_t* off_out) {
  size_t off = (m->blob_floats + 63) & ~(size_t)63;
  m->index[name] = {off, numel};
  m->blob_floats = off + numel;
  if (off_out) *off_out = off;
}

static int build_layout(ttx_model* m) {
  const ttx_config& c = m->cfg;
  const size_t d = c.embedding_dim, F = c.feedforward_dim, V = c.vocab_size, Vs = c.src_vocab_size;
  if (c.embedding_dim <= 0 || c.embedding_dim % 64 || c.embedding_dim > 1024)
    return fail(TTX_ERR_INVALID, "embedding_dim must be a multiple of 64 in [64,1024]");
  if (c.num_heads <= 0 || c.embedding_dim % c.num_heads || (c.embedding_dim / c.num_heads != 32 && c.embedding_dim / c.num_heads != 64))
    return fail(TTX_ERR_INVALID, "embedding_dim / num_heads must be 32 or 64");
  const int vpl = c.embedding_dim / 64;
  if (vpl != 1 && vpl != 2 && vpl != 4 && vpl != 8 && vpl != 16)
    return fail(TTX_ERR_INVALID, "embedding_dim must be 64, 128, 256, 512 or 1024");
  if (c.feedforward_dim <= 0 || c.feedforward_dim % 64) return fail(TTX_ERR_INVALID, "feedforward_dim must be a multiple of 64");
  if (c.vocab_size <= 0 || c.src_vocab_size <= 0) return fail(TTX_ERR_INVALID, "vocab sizes must be positive");
  if (c.num_encoder_layers <= 0 || c.num_decoder_layers <= 0) return fail(TTX_ERR_INVALID, "layer counts must be positive");
  if (c.max_positions <= 0) return fail(TTX_ERR_INVALID, "max_positions must be positive");

  auto attn = [&](const std::string& p, size_t* iw, size_t* ib, size_t* ow, size_t* ob) {
    layout_add(m, p + ".in_proj_weight", 3 * d * d, iw);
    layout_add(m, p + ".in_proj_bias", 3 * d, ib);
    layout_add(m, p + ".out_proj.weight", d * d, ow);
    layout_add(m, p + ".out_proj.bias", d, ob);
  };
  auto ffn = [&](const std::string& p, LayerW& w) {
    layout_add(m, p + ".linear1.weight", F * d, &w.l1_w);
    layout_add(m, p + ".linear1.bias", F, &w.l1_b);
    layout_add(m, p + ".linear2.weight", d * F, &w.l2_w);
    layout_add(m, p + ".linear2.bias", d, &w.l2_b);
  };
  auto norm = [&](const std::string& p, size_t* w, size_t* b) {
    layout_add(m, p + ".weight", d, w);
    layout_add(m, p + ".bias", d, b);
  };
  layout_add(m, "src_token_featurizer.embedding.weight", Vs * d, &m->src_emb);
  layout_add(m, "tgt_token_featurizer.embedding.weight", V * d, &m->tgt_emb);
  m->enc.resize(c.num_encoder_layers);
  for (int i = 0; i < c.num_encoder_layers; ++i) {
    const std::string p = "transformer.encoder.layers." + std::to_string(i);
    LayerW& w = m->enc[i];
    attn(p + ".self_attn", &w.sa_in_w, &w.sa_in_b, &w.sa_out_w, &w.sa_out_b);
    ffn(p, w);
    norm(p + ".norm1", &w.n1_w, &w.n1_b);
    norm(p + ".norm2", &w.n2_w, &w.n2_b);
  }
  norm("transformer.encoder.norm", &m->enc_norm_w, &m->enc_norm_b);
  m->dec.resize(c.num_decoder_layers);
  for (int i = 0; i < c.num_decoder_layers; ++i) {
    const std::string p = "transformer.decoder.layers." + std::to_string(i);
    LayerW& w = m->dec[i];
    attn(p + ".self_attn", &w.sa_in_w, &w.sa_in_b, &w.sa_out_w, &w.sa_out_b);
    attn(p + ".multihead_attn", &w.ca_in_w, &w.ca_in_b, &w.ca_out_w, &w.ca_out_b);
    ffn(p, w);
    norm(p + ".norm1", &w.n1_w, &w.n1_b);
    norm(p + ".norm2", &w.n2_w, &w.n2_b);
    norm(p + ".norm3", &w.n3_w, &w.n3_b);
  }
  norm("transformer.decoder.norm", &m->dec_norm_w, &m->dec_norm_b);
  layout_add(m, "next_token_classifier.weight", V * d, &m->cls_w);
  layout_add(m, "next_token_classifier.bias", V, &m->cls_b);
  // derived tensors (not in the state dict)
  layout_add(m, "positional_encoding.pe", ((size_t)c.max_positions + 1) * d, &m->pe);
  layout_add(m, "derived.cross_kv.weight", (size_t)c.num_decoder_layers * 2 * d * d, &m->cross_kv_w);
  layout_add(m, "derived.cross_kv.bias", (size_t)c.num_decoder_layers * 2 * d, &m->cross_kv_b);
  m->blob_floats = (m->blob_floats + 63) & ~(size_t)63;
  return TTX_OK;
}

static bool is_gfx950(int device) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return false;
  return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

extern "C" int ttx_abi_version(void) { return TTX_ABI_VERSION; }
extern "C" const char* ttx_last_error(void) { return g_err.c_str(); }

extern "C" int ttx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < n; ++i) ok += is_gfx950(i) ? 1 : 0;
  return ok;
}

static int model_alloc(const ttx_config* cfg, int device, ttx_model** out) {
  if (!cfg || !out) return fail(TTX_ERR_INVALID, "null argument");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(TTX_ERR_NO_DEVICE, "no HIP device visible; libttx_hip has no CPU fallback");
  if (device < 0 || device >= n) return fail(TTX_ERR_INVALID, "device index out of range");
  if (!is_gfx950(device)) return fail(TTX_ERR_NO_DEVICE, "device is not gfx950 (MI355X); this library is built for gfx950 only");
  ttx_model* m = new ttx_model();
  m->cfg = *cfg;
  m->device = device;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) m->n_cu = prop.multiProcessorCount;
  }
  int r = build_layout(m);
  if (r != TTX_OK) { delete m; return r; }
  if (hipSetDevice(device) != hipSuccess || hipMalloc(&m->blob, m->blob_floats * sizeof(float)) != hipSuccess) {
    delete m;
    return fail(TTX_ERR_NOMEM, "hipMalloc of the weight blob failed");
  }
  *out = m;
  return TTX_OK;
}

extern "C" int ttx_model_create_empty(const ttx_config* cfg, int device, ttx_model** out) {
  return model_alloc(cfg, device, out);
}

extern "C" int ttx_model_set_activation(ttx_model* m, int activation) {
  if (!m) return fail(TTX_ERR_INVALID, "null argument");
  if (activation != TTX_ACT_RELU && activation != TTX_ACT_GELU)
    return fail(TTX_ERR_INVALID, "the feed-forward activation is TTX_ACT_RELU or TTX_ACT_GELU");
  // captured graphs and step argument blocks of a session bake the FFN1 epilogue in
  if (m->n_sessions > 0) return fail(TTX_ERR_INVALID, "ttx_model_set_activation: the model already has had a session");
  m->activation = activation;
  return TTX_OK;
}

extern "C" int ttx_model_activation(const ttx_model* m) { return m ? m->activation : TTX_ACT_NONE; }

extern "C" int ttx_model_blob(ttx_model* m, void** d_ptr, int64_t* bytes) {
  if (!m || !d_ptr || !bytes) return fail(TTX_ERR_INVALID, "null argument");
  *d_ptr = m->blob;
  *bytes = (int64_t)(m->blob_floats * sizeof(float));
  return TTX_OK;
}

extern "C" int ttx_model_create(const ttx_config* cfg, const ttx_tensor* tensors, int n_tensors, int device,
                                ttx_model** out) {
  if (!tensors || n_tensors <= 0) return fail(TTX_ERR_INVALID, "no tensors given");
  ttx_model* m = nullptr;
  TTX_TRY(model_alloc(cfg, device, &m));
  std::vector<float> host(m->blob_floats, 0.f);
  std::map<std::string, const ttx_tensor*> given;
  for (int i = 0; i < n_tensors; ++i) {
    if (!tensors[i].name || !tensors[i].data) { ttx_model_destroy(m); return fail(TTX_ERR_INVALID, "tensor with null name/data"); }
    std::string nm = tensors[i].name;
    if (nm.rfind("model.", 0) == 0) nm = nm.substr(6);  // Lightning checkpoint prefix
    given[nm] = &tensors[i];
  }
  for (auto& kv : m->index) {
    const std::string& nm = kv.first;
    const bool derived = nm.rfind("derived.", 0) == 0;
    auto it = given.find(nm);
    if (it == given.end()) {
      if (derived || nm == "positional_encoding.pe") continue;
      ttx_model_destroy(m);
      return fail(TTX_ERR_INVALID, "missing tensor: " + nm);
    }
    if ((size_t)it->second->numel != kv.second.second) {
      ttx_model_destroy(m);
      return fail(TTX_ERR_INVALID, "tensor " + nm + " has " + std::to_string(it->second->numel) + " elements, expected " +
                                       std::to_string(kv.second.second));
    }
    std::memcpy(host.data() + kv.second.first, it->second->data, kv.second.second * sizeof(float));
  }
  const ttx_config& c = m->cfg;
  const size_t d = c.embedding_dim;
  if (given.find("positional_encoding.pe") == given.end()) {
    // embeddings.py:38-45 in fp32: row 0 zeros, row p+1 = sin/cos(p * exp(2i * (-ln 1e4 / d)))
    float* pe = host.data() + m->pe;
    const float cst = (float)(-std::log(10000.0) / (double)d);
    for (int p = 0; p < c.max_positions; ++p)
      for (size_t i = 0; i < d; i += 2) {
        const float div = expf((float)i * cst);
        const float arg = (float)p * div;
        pe[(size_t)(p + 1) * d + i] = sinf(arg);
        pe[(size_t)(p + 1) * d + i + 1] = cosf(arg);
      }
  }
  for (int l = 0; l < c.num_decoder_layers; ++l) {
    // rows d..3d of multihead_attn.in_proj_weight are the K and V projections (torch MHA packing)
    std::memcpy(host.data() + m->cross_kv_w + (size_t)l * 2 * d * d, host.data() + m->dec[l].ca_in_w + d * d, 2 * d * d * sizeof(float));
    std::memcpy(host.data() + m->cross_kv_b + (size_t)l * 2 * d, host.data() + m->dec[l].ca_in_b + d, 2 * d * sizeof(float));
  }
  if (hipMemcpy(m->blob, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    ttx_model_destroy(m);
    return fail(TTX_ERR_HIP, "hipMemcpy of the weight blob failed");
  }
  *out = m;
  return TTX_OK;
}

extern "C" void ttx_model_destroy(ttx_model* m) {
  if (!m) return;
  if (m->blob) (void)hipFree(m->blob);
  delete m;
}

// Growing a workspace must not stall the other sessions' streams: hipFree waits for the whole device, so the old
// allocation is parked here and released at the start of a later top-level call (or when a session is destroyed),
// when nothing of the previous call is in flight any more.  Work already enqueued keeps using the old allocation;
// whatever is enqueued after the growth uses the new one (workspaces carry no state across a growth).
static std::mutex g_retired_mu;
static std::vector<void*> g_retired;

static void release_retired() {
  std::vector<void*> v;
  {
    std::lock_guard<std::mutex> lk(g_retired_mu);
    v.swap(g_retired);
  }
  if (v.empty()) return;
  (void)hipDeviceSynchronize();
  for (void* p : v) (void)hipFree(p);
}

// Session streams come from a per-device cache that outlives the sessions.  The runtime binds a stream to one of its few
// hardware queues when the stream is created, round-robin over every stream the process ever made: the streams of a SECOND
// model's sessions (after the first model was closed) landed two to a queue and its pools ran 7 % slower than in a fresh process
// (tools/exp/inline_order.py, profiles/r03_stream_reuse.txt).  Handing the same streams out again, lowest creation index first,
// gives every later set of sessions the queue layout of the first.
static std::mutex g_stream_mu;
static std::map<int, std::vector<std::pair<int, hipStream_t>>> g_free_streams;      // device -> (creation index, stream), idle
static std::map<hipStream_t, int> g_stream_index;
static int g_streams_made = 0;

static int ensure_own_stream(ttx_session* s) {
  if (s->own_stream) return TTX_OK;
  std::lock_guard<std::mutex> lock(g_stream_mu);
  auto& idle = g_free_streams[s->m->device];
  if (!idle.empty()) {
    auto it = std::min_element(idle.begin(), idle.end());
    s->own_stream = it->second;
    idle.erase(it);
    return TTX_OK;
  }
  HIP_TRY(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
  g_stream_index[s->own_stream] = g_streams_made++;
  return TTX_OK;
}

static void release_own_stream(ttx_session* s) {        // the stream is idle (the caller synchronised the device)
  if (!s->own_stream) return;
  std::lock_guard<std::mutex> lock(g_stream_mu);
  g_free_streams[s->m->device].push_back({g_stream_index[s->own_stream], s->own_stream});
  s->own_stream = nullptr;
}

static int ensure(Buf& b, size_t bytes, hipStream_t st) {
  (void)st;
  if (bytes <= b.cap) return TTX_OK;
  if (b.owner_gen) ++*b.owner_gen;
  if (b.p) {
    std::lock_guard<std::mutex> lk(g_retired_mu);
    g_retired.push_back(b.p);
    b.p = nullptr;
    b.cap = 0;
  }
  size_t want = bytes + bytes / 8 + 256;
  if (hipMalloc(&b.p, want) != hipSuccess) return fail(TTX_ERR_NOMEM, "hipMalloc failed for " + std::to_string(want) + " bytes");
  b.cap = want;
  // TTX_POISON_WORKSPACES=1 (tests): fresh workspaces are filled with 0xFF bytes (NaN as floats, -1 as ints), so that
  // any dependence on never-written workspace memory shows up deterministically instead of once in a while
  static const bool poison = getenv("TTX_POISON_WORKSPACES") != nullptr && atoi(getenv("TTX_POISON_WORKSPACES")) != 0;
  if (poison) {
    if (hipMemset(b.p, 0xFF, want) != hipSuccess) return fail(TTX_ERR_HIP, "hipMemset (poison) failed");
    (void)hipDeviceSynchronize();
  }
  return TTX_OK;
}

extern "C" int ttx_session_create(ttx_model* m, ttx_session** out) {
  if (!m || !out) return fail(TTX_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(m->device));
  ttx_session* s = new ttx_session();
  s->m = m;
  if (hipHostMalloc((void**)&s->host_info, sizeof(HostInfo), hipHostMallocMapped) != hipSuccess ||
      hipHostMalloc((void**)&s->probe_info, sizeof(ProbeInfo), hipHostMallocMapped) != hipSuccess ||
      hipHostMalloc((void**)&s->host_state, sizeof(DecState), hipHostMallocDefault) != hipSuccess) {
    if (s->host_info) (void)hipHostFree(s->host_info);
    if (s->probe_info) (void)hipHostFree(s->probe_info);
    if (s->host_state) (void)hipHostFree(s->host_state);
    delete s;
    return fail(TTX_ERR_NOMEM, "hipHostMalloc failed");
  }
  std::memset(s->host_info, 0, sizeof(HostInfo));
  std::memset(s->probe_info, 0, sizeof(ProbeInfo));
  HIP_TRY(hipEventCreate(&s->ev_a));
  HIP_TRY(hipEventCreate(&s->ev_b));
  HIP_TRY(hipEventCreate(&s->ev_c));
  HIP_TRY(hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming));
  s->use_graphs = getenv("TTX_NO_GRAPH") == nullptr;
  const char* pf = getenv("TTX_PROFILE_GEMM");
  s->profile = pf && pf[0] == '1';
  // tuning knob: the live row count below which a step takes the short-chain GEMM variant (identical bits)
  if (const char* e = getenv("TTX_SMALL_ROWS")) s->small_rows = std::max(0, atoi(e));
  if (const char* e = getenv("TTX_FFN2_SLAB_ROWS")) s->ffn2_slab_rows = std::max(0, atoi(e));
  if (const char* e = getenv("TTX_QKV_SMALL_ROWS")) s->qkv_small_rows = std::max(0, atoi(e));
  // test hook: every attention launch on the streaming fallback kernel
  if (const char* e = getenv("TTX_ATTN_FALLBACK")) s->attn_fallback = atoi(e) != 0;
  if (const char* e = getenv("TTX_ACCEPT_SPREAD")) s->accept_spread = atoi(e) != 0;
  // A/B and test switch: 0 keeps one-row step launches off k_attn1, 1 puts every eligible one on it
  if (const char* e = getenv("TTX_ATTN_ROW")) s->attn_row = atoi(e) != 0 ? 1 : 0;
  s->host_timing = getenv("TTX_HOST_TIMING") != nullptr;
  m->n_sessions++;                                   // from here on the model's activation is fixed (ttx_model_set_activation)
  *out = s;
  return TTX_OK;
}

extern "C" void ttx_session_destroy(ttx_session* s) {
  if (!s) return;
  if (s->host_timing && s->host_launches)
    fprintf(stderr, "[ttx host timing] hipGraphLaunch: %lld launches, %.1f us each\n", s->host_launches,
            s->host_launch_us / (double)s->host_launches);
  if (s->host_timing && s->host_captures)
    fprintf(stderr, "[ttx host timing] graphs captured: %lld, %.1f us each\n", s->host_captures,
            s->host_capture_us / (double)s->host_captures);
  if (s->dead) {        // hipFree / hipDeviceSynchronize would wait for the stuck stream, and a late kernel may still write
    delete s;           // the mapped host words: leak workspaces, pinned memory, graphs and events of a hung session
    return;
  }
  release_retired();
  (void)hipDeviceSynchronize();
  for (Buf* b : s->all)
    if (b->p) (void)hipFree(b->p);
  if (s->host_info) (void)hipHostFree(s->host_info);
  if (s->probe_info) (void)hipHostFree(s->probe_info);
  if (s->beam_host) (void)hipHostFree(s->beam_host);
  if (s->bp_host) (void)hipHostFree(s->bp_host);
  s->drop_graphs();
  release_own_stream(s);
  if (s->ev_done) (void)hipEventDestroy(s->ev_done);
  if (s->host_state) (void)hipHostFree(s->host_state);
  for (auto& e : s->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  if (s->ev_a) (void)hipEventDestroy(s->ev_a);
  if (s->ev_b) (void)hipEventDestroy(s->ev_b);
  if (s->ev_c) (void)hipEventDestroy(s->ev_c);
  delete s;
}

// ------------------------------------------------------------------------------------------------
// GEMM variant of a launch (ttx_internal.h: all variants return identical bits).  Steps: by live rows; bulk passes
// (encoder, cross K/V, full-prefix decoder) by their row count.
static int variant_for_rows(const ttx_session* s, long long rows, bool step) {
  if (!step) return GV_BIG;
  if (rows < s->qkv_small_rows) return GV_SMALL;
  if (rows < s->small_rows) return GV_MID;
  return rows < s->ffn2_slab_rows ? GV_BIG_FFN2_SLABS : GV_BIG;
}
// the step policy per GEMM shape (ttx_internal.h): QKV (N = 3d) | the d-wide K = d GEMMs and the classifier | FFN1 | FFN2
static int variant_qkv(int v) { return v == GV_SMALL ? GV_SMALL : GV_BIG; }
static int variant_dd(int v) { return (v == GV_SMALL || v == GV_MID) ? GV_SMALL : GV_BIG; }
static int variant_ffn1(int v) { return v == GV_SMALL ? GV_SMALL : GV_BIG; }
static int variant_ffn2(int v) { return v == GV_BIG ? GV_BIG : GV_SMALL; }

// d-wide GEMM -> slab(s) -> k_finish_ln: Y = LN2?(LN((resid + bias) + X W^T))
static int gemm_ln(ttx_session* s, hipStream_t st, const float* X, int ldx, int K, const float* W, const float* bias,
                   const float* resid, const float* g1, const float* b1, const float* g2, const float* b2,
                   const uint8_t* row_valid, float* Y, const int* m_ptr, int Mmax, int variant) {
  const int d = s->m->cfg.embedding_dim;
  const int S = gemm_splits(d, K, m_ptr != nullptr, variant);
  const long long stride = (long long)Mmax * d;
  TTX_TRY(ensure(s->slab, sizeof(float) * (size_t)S * stride, st));
  TTX_TRY(launch_gemm(s, st, X, ldx, W, K, nullptr, s->slab.as<float>(), d, m_ptr, Mmax, d, K, false, S, stride, variant));
  return launch_finish(s, st, s->slab.as<float>(), S, stride, bias, resid, g1, b1, g2, b2, row_valid, Y, m_ptr, Mmax);
}

// The feed-forward half of a layer on the rows in `x`: Y = LN2?(LN(x + b2 + act(x W1^T + b1) W2^T)), LN from the layer's norm at
// (n_w, n_b), LN2 (g2, b2: the stack's final norm, null except behind its last layer); rows with row_valid[row] == 0 come out zero.
static int ffn_half(ttx_session* s, hipStream_t st, const LayerW& w, const float* x, size_t n_w, size_t n_b, const float* g2,
                    const float* b2, const uint8_t* row_valid, float* Y, const int* m_ptr, int Mmax, int v_ffn1, int v_ffn2) {
  const ttx_model* m = s->m;
  const int d = m->cfg.embedding_dim, F = m->cfg.feedforward_dim;
  float* hb = s->hbuf.as<float>();
  TTX_TRY(launch_gemm(s, st, x, d, m->p(w.l1_w), d, m->p(w.l1_b), hb, F, m_ptr, Mmax, F, d, m->activation, 0, 0, v_ffn1));
  return gemm_ln(s, st, hb, F, F, m->p(w.l2_w), m->p(w.l2_b), x, m->p(n_w), m->p(n_b), g2, b2, row_valid, Y, m_ptr, Mmax, v_ffn2);
}

static int ensure_acts(ttx_session* s, hipStream_t st, size_t M, int qkv_layers) {
  const ttx_config& c = s->m->cfg;
  const size_t d = c.embedding_dim, F = c.feedforward_dim;
  TTX_TRY(ensure(s->x, M * d * 4, st));
  TTX_TRY(ensure(s->x1, M * d * 4, st));
  TTX_TRY(ensure(s->x2, M * d * 4, st));
  TTX_TRY(ensure(s->xf, M * d * 4, st));
  TTX_TRY(ensure(s->ao, M * d * 4, st));
  TTX_TRY(ensure(s->q2, M * d * 4, st));
  TTX_TRY(ensure(s->hbuf, M * F * 4, st));
  TTX_TRY(ensure(s->qkv, (size_t)qkv_layers * M * 3 * d * 4, st));
  return TTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Encoder: tokens int32 [B*Ls] + valid mask -> memory [B*Ls, d] (zeros at PAD rows).  modules.py:110-116
// `qkv_buf`: where the encoder keeps its packed Q/K/V rows (default: the session's step buffer — callers whose NEXT step still
// needs the previous step's Q/K/V rows, i.e. the beam source pool's deferred cache hand-over, pass a buffer of their own).
static int run_encoder(ttx_session* s, hipStream_t st, const int* tok, const uint8_t* valid, int B, int Ls, float* memory,
                       float* qkv_buf = nullptr) {
  const ttx_model* m = s->m;
  const ttx_config& c = m->cfg;
  const int d = c.embedding_dim, H = c.num_heads;
  const int M = B * Ls;
  const int gv = variant_for_rows(s, M, false);
  TTX_TRY(ensure_acts(s, st, (size_t)M, 1));
  float* x = s->x.as<float>();
  float* x1 = s->x1.as<float>();
  float* qkv = qkv_buf ? qkv_buf : s->qkv.as<float>();
  float* ao = s->ao.as<float>();
  EmbedArgs e{};
  e.table = m->p(m->src_emb); e.pe = m->p(m->pe); e.X = x; e.d = d; e.V = c.src_vocab_size; e.tok = tok; e.rows = M; e.L = Ls;
  hipLaunchKernelGGL((k_embed<false>), dim3(cdiv(M, 4)), dim3(256), 0, st, e);
  HIP_TRY(hipGetLastError());
  for (int l = 0; l < c.num_encoder_layers; ++l) {
    const LayerW& w = m->enc[l];
    const bool last = (l == c.num_encoder_layers - 1);
    TTX_TRY(launch_gemm(s, st, x, d, m->p(w.sa_in_w), d, m->p(w.sa_in_b), qkv, 3 * d, nullptr, M, 3 * d, d, false, 0, 0, gv));
    AttnArgs a{};
    a.q = qkv; a.ldq = 3 * d; a.k = qkv + d; a.v = qkv + 2 * d; a.ldkv = 3 * d; a.out = ao; a.d = d;
    a.scale = 1.0f / sqrtf((float)(d / H)); a.L = Ls; a.tok = tok; a.pad = c.pad_token;
    TTX_TRY(launch_attn(ATT_ENC, s, st, a, B, H, Ls, Ls));
    TTX_TRY(gemm_ln(s, st, ao, d, d, m->p(w.sa_out_w), m->p(w.sa_out_b), x, m->p(w.n1_w), m->p(w.n1_b), nullptr, nullptr,
                    nullptr, x1, nullptr, M, gv));
    TTX_TRY(ffn_half(s, st, w, x1, w.n2_w, w.n2_b, last ? m->p(m->enc_norm_w) : nullptr, last ? m->p(m->enc_norm_b) : nullptr,
                     last ? valid : nullptr, last ? memory : x, nullptr, M, gv, gv));
  }
  return TTX_OK;
}

static int prepare_tokens(hipStream_t st, const int64_t* d_in, int* out, uint8_t* valid, int n, int pad) {
  hipLaunchKernelGGL(k_prepare_tokens, dim3(cdiv(n, 256)), dim3(256), 0, st, d_in, out, valid, n, pad);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// The sources of a decoding loop: R rows of Ls int64 tokens at d_src (ld_src apart; 0: packed, B x Ls in one piece) -> s->tok_src
// and `valid`, the encoder into s->memory, and the cross-attention K/V of every decoder layer, packed [R * Ls][Ld * 2d], into
// `memkv`.  enc_qkv: run_encoder's qkv_buf.
static int encode_sources(ttx_session* s, hipStream_t st, const int64_t* d_src, int ld_src, int R, int Ls, uint8_t* valid, float* memkv,
                          float* enc_qkv = nullptr) {
  const ttx_model* m = s->m;
  const int d = m->cfg.embedding_dim, kv_row = m->cfg.num_decoder_layers * 2 * d;
  if (ld_src == 0) {
    TTX_TRY(prepare_tokens(st, d_src, s->tok_src.as<int>(), valid, R * Ls, m->cfg.pad_token));
  } else {
    hipLaunchKernelGGL(k_prepare_tokens_2d, dim3(cdiv(R * Ls, 256)), dim3(256), 0, st, d_src, ld_src, s->tok_src.as<int>(), valid, R, Ls,
                       m->cfg.pad_token);
    HIP_TRY(hipGetLastError());
  }
  TTX_TRY(run_encoder(s, st, s->tok_src.as<int>(), valid, R, Ls, s->memory.as<float>(), enc_qkv));
  return launch_gemm(s, st, s->memory.as<float>(), d, m->p(m->cross_kv_w), d, m->p(m->cross_kv_b), memkv, kv_row, nullptr, R * Ls, kv_row,
                     d, false, 0, 0, variant_for_rows(s, (long long)R * Ls, false));
}

// Sizes the workspaces of a call before anything is enqueued or captured: need(buffer, bytes) for each, then TTX_TRY(need.rc).
// The first failure sticks and skips the rest.
struct Needs {
  hipStream_t st;
  int rc = TTX_OK;
  void operator()(Buf& b, size_t bytes) { if (rc == TTX_OK) rc = ensure(b, bytes, st); }
};

// What every decoding loop needs for its verify steps of up to Mmax rows, next to an encoder pass over src_rows rows: the argmax,
// the loop state, the logits, and the activation, Q/K/V and slab buffers the encoder and the step share (sized for the larger).
static void need_step_workspaces(ttx_session* s, Needs& need, size_t Mmax, size_t src_rows) {
  const ttx_config& c = s->m->cfg;
  const size_t d = c.embedding_dim, Macts = std::max(Mmax, src_rows);
  need(s->pred, Mmax * 4); need(s->state, sizeof(DecState)); need(s->logits, Mmax * c.vocab_size * 4);
  if (need.rc == TTX_OK) need.rc = ensure_acts(s, need.st, Macts, 1);
  need(s->qkv, std::max((size_t)c.num_decoder_layers * Mmax, src_rows) * 3 * d * 4);
  need(s->slab, sizeof(float) * 16 * Macts * d);            // no allocation may happen inside a graph capture
}

// The source side of a pool of C slots of Ls_cap positions: the staging buffers of an admission and the slots' own copies.
static void need_source_slots(ttx_session* s, Needs& need, int C, int Ls_cap) {
  const ttx_config& c = s->m->cfg;
  const size_t rows = (size_t)C * Ls_cap, kv_row = (size_t)c.num_decoder_layers * 2 * c.embedding_dim;
  need(s->tok_src, rows * 4); need(s->valid_new, rows); need(s->src_valid, rows);
  need(s->memory, rows * c.embedding_dim * 4); need(s->memkv_new, rows * kv_row * 4); need(s->memkv, rows * kv_row * 4);
}

extern "C" int ttx_encode_src(ttx_session* s, const int64_t* d_src, int B, int Ls, float* d_memory, void* stream) {
  if (!s || !d_src || !d_memory || B <= 0 || Ls <= 0) return fail(TTX_ERR_INVALID, "bad argument to ttx_encode_src");
  if (Ls > s->m->cfg.max_positions) return fail(TTX_ERR_INVALID, "source longer than the positional table");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  TTX_TRY(ensure(s->tok_src, (size_t)B * Ls * 4, st));
  TTX_TRY(ensure(s->src_valid, (size_t)B * Ls, st));
  TTX_TRY(prepare_tokens(st, d_src, s->tok_src.as<int>(), s->src_valid.as<uint8_t>(), B * Ls, s->m->cfg.pad_token));
  return run_encoder(s, st, s->tok_src.as<int>(), s->src_valid.as<uint8_t>(), B, Ls, d_memory);
}

// ------------------------------------------------------------------------------------------------
// The rows one pass of the decoder stack runs on: a bulk pass over M rows (m_ptr null, Mmax = M, every variant GV_BIG, one
// Q/K/V buffer for all layers) or a verify step (live row count on the device, per-shape variants, Q/K/V rows kept per layer).
struct StackRows {
  const int* m_ptr;
  int Mmax;
  int v_qkv, v_dd, v_ffn1, v_ffn2;   // GemmVariant per GEMM shape: QKV | the d-wide K = d GEMMs and the classifier | FFN1 | FFN2
  float* qkv;                        // layer l's packed Q/K/V rows start at qkv + l * qkv_layer
  long long qkv_layer;
};

// Decoder layers and classifier over the embedded rows in s->x: per layer QKV GEMM, self attention, out-projection + LN, Q GEMM,
// cross attention, out-projection + LN, feed-forward (+ the final norm behind the last layer); then logits = classifier(xf).
// self_attn(l, qkv) and cross_attn(l) launch layer l's attention from the layer's Q/K/V rows / from s->q2 into s->ao.
// stop_layer >= 0: the pass ends behind cross_attn(stop_layer) (the cross-attention tap: nothing downstream of s->q2 is wanted).
template <class SelfAttn, class CrossAttn>
static int run_decoder_stack(ttx_session* s, hipStream_t st, const StackRows& r, SelfAttn&& self_attn, CrossAttn&& cross_attn,
                             float* logits, int stop_layer = -1) {
  const ttx_model* m = s->m;
  const ttx_config& c = m->cfg;
  const int d = c.embedding_dim, V = c.vocab_size, Ld = c.num_decoder_layers;
  float* x = s->x.as<float>();
  float* x1 = s->x1.as<float>();
  float* x2 = s->x2.as<float>();
  float* xf = s->xf.as<float>();
  float* ao = s->ao.as<float>();
  float* q2 = s->q2.as<float>();
  for (int l = 0; l < Ld; ++l) {
    const LayerW& w = m->dec[l];
    const bool last = (l == Ld - 1);
    float* qkv = r.qkv + (size_t)l * r.qkv_layer;
    TTX_TRY(launch_gemm(s, st, x, d, m->p(w.sa_in_w), d, m->p(w.sa_in_b), qkv, 3 * d, r.m_ptr, r.Mmax, 3 * d, d, false, 0, 0, r.v_qkv));
    TTX_TRY(self_attn(l, qkv));
    TTX_TRY(gemm_ln(s, st, ao, d, d, m->p(w.sa_out_w), m->p(w.sa_out_b), x, m->p(w.n1_w), m->p(w.n1_b), nullptr, nullptr,
                    nullptr, x1, r.m_ptr, r.Mmax, r.v_dd));
    TTX_TRY(launch_gemm(s, st, x1, d, m->p(w.ca_in_w), d, m->p(w.ca_in_b), q2, d, r.m_ptr, r.Mmax, d, d, false, 0, 0, r.v_dd));
    TTX_TRY(cross_attn(l));
    if (l == stop_layer) return TTX_OK;
    TTX_TRY(gemm_ln(s, st, ao, d, d, m->p(w.ca_out_w), m->p(w.ca_out_b), x1, m->p(w.n2_w), m->p(w.n2_b), nullptr, nullptr,
                    nullptr, x2, r.m_ptr, r.Mmax, r.v_dd));
    TTX_TRY(ffn_half(s, st, w, x2, w.n3_w, w.n3_b, last ? m->p(m->dec_norm_w) : nullptr, last ? m->p(m->dec_norm_b) : nullptr,
                     nullptr, last ? xf : x, r.m_ptr, r.Mmax, r.v_ffn1, r.v_ffn2));
  }
  return launch_gemm(s, st, xf, d, m->p(m->cls_w), d, m->p(m->cls_b), logits, V, r.m_ptr, r.Mmax, V, d, false, 0, 0, r.v_dd);
}

// The cross-attention tap of run_decoder_full: the probabilities of decoder layer `layer` (csrc/ttx_attn_probs.hip.h).
struct AttnTap {
  int layer;
  const int* length;                 // [R]: query position t of row r is live iff t < length[r]
  float* heads;                      // [R, H, Lt, Ls] or null
  float* mean;                       // [R, Lt, Ls] or null
  int* align;                        // [R, Lt] or null
};

static int launch_attn_probs(ttx_session* s, hipStream_t st, const AttnProbsArgs& a, int head_dim);

// Full-prefix decoder (modules.py:118-138).  tok int32 [R*Lt]; memory fp32 [Rm*Ls, d]; mem_pad u8 [Rm*Ls].  With a tap the pass
// ends at the tapped layer's cross attention: its K projection of the memory, its Q projection, k_attn_probs, and nothing after
// (logits are not formed); without one the launches are the same as ever.
static int run_decoder_full(ttx_session* s, hipStream_t st, const int* tok, int R, int Lt, const float* memory,
                            const uint8_t* mem_pad, const int* mem_row, int Rm, int Ls, float* logits,
                            const AttnTap* tap = nullptr) {
  const ttx_model* m = s->m;
  const ttx_config& c = m->cfg;
  const int d = c.embedding_dim, H = c.num_heads;
  const int M = R * Lt, Mk = Rm * Ls;
  const int gv = variant_for_rows(s, M, false);
  TTX_TRY(ensure_acts(s, st, (size_t)M, 1));
  TTX_TRY(ensure(s->ckv, (size_t)Mk * 2 * d * 4, st));
  float* ao = s->ao.as<float>();
  float* ckv = s->ckv.as<float>();
  const float scale = 1.0f / sqrtf((float)(d / H));
  EmbedArgs e{};
  e.table = m->p(m->tgt_emb); e.pe = m->p(m->pe); e.X = s->x.as<float>(); e.d = d; e.V = c.vocab_size; e.tok = tok; e.rows = M; e.L = Lt;
  hipLaunchKernelGGL((k_embed<false>), dim3(cdiv(M, 4)), dim3(256), 0, st, e);
  HIP_TRY(hipGetLastError());
  const StackRows rows{nullptr, M, gv, gv, gv, gv, s->qkv.as<float>(), 0};
  return run_decoder_stack(s, st, rows,
      [&](int, float* qkv) -> int {
        AttnArgs a{};
        a.q = qkv; a.ldq = 3 * d; a.k = qkv + d; a.v = qkv + 2 * d; a.ldkv = 3 * d; a.out = ao; a.d = d; a.scale = scale;
        a.L = Lt; a.tok = tok; a.pad = c.pad_token;
        return launch_attn(ATT_FULL_SELF, s, st, a, R, H, Lt, Lt);
      },
      [&](int l) -> int {
        // cross attention: Q from the decoder stream, K/V re-projected from `memory` (as the reference does per call)
        const LayerW& w = m->dec[l];
        TTX_TRY(launch_gemm(s, st, memory, d, m->p(w.ca_in_w) + (size_t)d * d, d, m->p(w.ca_in_b) + d, ckv, 2 * d, nullptr, Mk,
                            2 * d, d, false, 0, 0, gv));
        if (tap && l == tap->layer) {
          AttnProbsArgs pa{};
          pa.q = s->q2.as<float>(); pa.ldq = d; pa.k = ckv; pa.ldkv = 2 * d; pa.key_pad = mem_pad; pa.mem_row = mem_row;
          pa.length = tap->length; pa.heads = tap->heads; pa.mean = tap->mean; pa.align = tap->align;
          pa.R = R; pa.Rm = Rm; pa.H = H; pa.T = Lt; pa.Ls = Ls; pa.scale = scale;
          return launch_attn_probs(s, st, pa, d / H);
        }
        AttnArgs ca{};
        ca.q = s->q2.as<float>(); ca.ldq = d; ca.k = ckv; ca.v = ckv + d; ca.ldkv = 2 * d; ca.out = ao; ca.d = d; ca.scale = scale;
        ca.L = Lt; ca.Lk = Ls; ca.key_pad = mem_pad; ca.mem_row = mem_row;
        return launch_attn(ATT_FULL_CROSS, s, st, ca, R, H, Lt, Ls);
      },
      logits, tap ? tap->layer : -1);
}

extern "C" int ttx_decode_tgt(ttx_session* s, const int64_t* d_tgt, int R, int Lt, const float* d_memory,
                              const uint8_t* d_mem_pad, const int32_t* d_mem_row, int Rm, int Ls, float* d_logits,
                              void* stream) {
  if (!s || !d_tgt || !d_memory || !d_mem_pad || !d_logits || R <= 0 || Lt <= 0 || Rm <= 0 || Ls <= 0)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_decode_tgt");
  if (!d_mem_row && Rm != R) return fail(TTX_ERR_INVALID, "without a row map the memory must have one row per decoder row");
  if (Lt > s->m->cfg.max_positions) return fail(TTX_ERR_INVALID, "target longer than the positional table");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  TTX_TRY(ensure(s->tok_tgt, (size_t)R * Lt * 4, st));
  TTX_TRY(prepare_tokens(st, d_tgt, s->tok_tgt.as<int>(), nullptr, R * Lt, s->m->cfg.pad_token));
  return run_decoder_full(s, st, s->tok_tgt.as<int>(), R, Lt, d_memory, d_mem_pad, d_mem_row, Rm, Ls, d_logits);
}

__global__ void k_invert_mask(const uint8_t* valid, uint8_t* pad, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pad[i] = valid[i] ? 0 : 1;
}

extern "C" int ttx_forward(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_tgt, int Lt,
                           float* d_logits, void* stream) {
  if (!s || !d_src || !d_tgt || !d_logits || B <= 0 || Ls <= 0 || Lt <= 0) return fail(TTX_ERR_INVALID, "bad argument to ttx_forward");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  const int d = s->m->cfg.embedding_dim;
  TTX_TRY(ensure(s->memory, (size_t)B * Ls * d * 4, st));
  TTX_TRY(ensure(s->mem_pad_tmp, (size_t)B * Ls, st));
  TTX_TRY(ttx_encode_src(s, d_src, B, Ls, s->memory.as<float>(), stream));
  hipLaunchKernelGGL(k_invert_mask, dim3(cdiv(B * Ls, 256)), dim3(256), 0, st, s->src_valid.as<uint8_t>(),
                     s->mem_pad_tmp.as<uint8_t>(), B * Ls);
  HIP_TRY(hipGetLastError());
  return ttx_decode_tgt(s, d_tgt, B, Lt, s->memory.as<float>(), s->mem_pad_tmp.as<uint8_t>(), nullptr, B, Ls, d_logits, stream);
}

// ------------------------------------------------------------------------------------------------
// Teacher-forced evaluation (lightning_model.py:174-207, metrics.py): csrc/ttx_metrics.hip.h.
static int session_required(const char* fn) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(TTX_ERR_NO_DEVICE, "no HIP device visible; libttx_hip has no CPU fallback");
  return fail(TTX_ERR_INVALID, std::string("bad argument to ") + fn + ": null session");
}

static int check_metric_shapes(const ttx_session* s, int B, int Lt, int V, const char* fn) {
  if (B <= 0 || Lt < 2 || V <= 0) return fail(TTX_ERR_INVALID, std::string("bad argument to ") + fn + ": B > 0, Lt >= 2, V > 0");
  if (V > MET_MAX_V) return fail(TTX_ERR_INVALID, std::string(fn) + ": vocabulary larger than 1024");
  if ((long long)B * (Lt - 1) >= (1LL << 24))      // token / sequence hit counts stay exact in fp32, as torch's float mean has them
    return fail(TTX_ERR_INVALID, std::string(fn) + ": more than 2^24 positions in one call");
  if (Lt - 1 > s->m->cfg.max_positions) return fail(TTX_ERR_INVALID, std::string(fn) + ": target longer than the positional table");
  return TTX_OK;
}

static int launch_metrics(ttx_session* s, hipStream_t st, const float* logits, const int64_t* tgt, int B, int Lt, int V, int eos,
                          int64_t* pred, float* nll, float* out3) {
  const int M = B * (Lt - 1);
  if (!pred) {
    TTX_TRY(ensure(s->ev_pred, (size_t)M * sizeof(int64_t), st));
    pred = s->ev_pred.as<int64_t>();
  }
  if (!nll) {
    TTX_TRY(ensure(s->ev_nll, (size_t)M * sizeof(float), st));
    nll = s->ev_nll.as<float>();
  }
  if (V % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0)
    hipLaunchKernelGGL(k_token_metrics<true>, dim3(cdiv(M, 4)), dim3(256), 0, st, logits, tgt, Lt, M, V, pred, nll);
  else
    hipLaunchKernelGGL(k_token_metrics<false>, dim3(cdiv(M, 4)), dim3(256), 0, st, logits, tgt, Lt, M, V, pred, nll);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_batch_metrics, dim3(1), dim3(MET_BATCH_THREADS), 0, st, pred, nll, tgt, B, Lt, eos, out3);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

extern "C" int ttx_token_metrics(ttx_session* s, const float* d_logits, const int64_t* d_tgt, int B, int Lt, int V, int eos,
                                 int64_t* d_pred, float* d_nll, float* d_out3, void* stream) {
  if (!s) return session_required("ttx_token_metrics");
  if (!d_logits || !d_tgt || !d_out3) return fail(TTX_ERR_INVALID, "bad argument to ttx_token_metrics");
  TTX_TRY(check_metric_shapes(s, B, Lt, V, "ttx_token_metrics"));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  return launch_metrics(s, st, d_logits, d_tgt, B, Lt, V, eos, d_pred, d_nll, d_out3);
}

extern "C" int ttx_teacher_forced_eval(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_tgt, int Lt, int eos,
                                       float* d_logits, int64_t* d_pred, float* d_nll, float* d_out3, void* stream) {
  if (!s) return session_required("ttx_teacher_forced_eval");
  if (!d_src || !d_tgt || !d_out3 || Ls <= 0) return fail(TTX_ERR_INVALID, "bad argument to ttx_teacher_forced_eval");
  const ttx_config& c = s->m->cfg;
  TTX_TRY(check_metric_shapes(s, B, Lt, c.vocab_size, "ttx_teacher_forced_eval"));
  if (Ls > c.max_positions) return fail(TTX_ERR_INVALID, "source longer than the positional table");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  const int T = Lt - 1, V = c.vocab_size, d = c.embedding_dim;
  if (!d_logits) {
    TTX_TRY(ensure(s->ev_logits, (size_t)B * T * V * sizeof(float), st));
    d_logits = s->ev_logits.as<float>();
  }
  // ttx_forward(src, tgt[:, :-1]) without a sliced copy: the decoder's int32 tokens are read off the [B, Lt] rows directly
  TTX_TRY(ensure(s->memory, (size_t)B * Ls * d * 4, st));
  TTX_TRY(ensure(s->mem_pad_tmp, (size_t)B * Ls, st));
  TTX_TRY(ttx_encode_src(s, d_src, B, Ls, s->memory.as<float>(), stream));
  hipLaunchKernelGGL(k_invert_mask, dim3(cdiv(B * Ls, 256)), dim3(256), 0, st, s->src_valid.as<uint8_t>(),
                     s->mem_pad_tmp.as<uint8_t>(), B * Ls);
  HIP_TRY(hipGetLastError());
  TTX_TRY(ensure(s->tok_tgt, (size_t)B * T * 4, st));
  hipLaunchKernelGGL(k_prepare_tokens_2d, dim3(cdiv(B * T, 256)), dim3(256), 0, st, d_tgt, Lt, s->tok_tgt.as<int>(),
                     (uint8_t*)nullptr, B, T, c.pad_token);
  HIP_TRY(hipGetLastError());
  TTX_TRY(run_decoder_full(s, st, s->tok_tgt.as<int>(), B, T, s->memory.as<float>(), s->mem_pad_tmp.as<uint8_t>(), nullptr, B, Ls,
                           d_logits));
  return launch_metrics(s, st, d_logits, d_tgt, B, Lt, V, eos, d_pred, d_nll, d_out3);
}

// ------------------------------------------------------------------------------------------------
// Log-likelihood scores of hypotheses: csrc/ttx_score.hip.h.
static int check_score_shapes(const ttx_session* s, long long R, int W, int V, const char* fn) {
  if (R <= 0 || W < 2 || V <= 0) return fail(TTX_ERR_INVALID, std::string("bad argument to ") + fn + ": rows > 0, W >= 2, V > 0");
  if (V > MET_MAX_V) return fail(TTX_ERR_INVALID, std::string(fn) + ": vocabulary larger than 1024");
  if (R * (W - 1) >= (1LL << 24)) return fail(TTX_ERR_INVALID, std::string(fn) + ": more than 2^24 positions in one call");
  if (W - 1 > s->m->cfg.max_positions) return fail(TTX_ERR_INVALID, std::string(fn) + ": hypothesis longer than the positional table");
  return TTX_OK;
}

static int launch_score(ttx_session* s, hipStream_t st, const float* logits, const int64_t* hyp, int ld_hyp, int R, int W, int V,
                        int pad, int eos, float* tok_logp, float* score, int32_t* length, uint8_t* finished) {
  if (!tok_logp) {                        // the sum reads the per-token values back: session scratch when the caller wants none
    TTX_TRY(ensure(s->ev_nll, (size_t)R * (W - 1) * sizeof(float), st));
    tok_logp = s->ev_nll.as<float>();
  }
  if (V % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0)
    hipLaunchKernelGGL(k_hyp_score<true>, dim3(R), dim3(SCORE_THREADS), 0, st, logits, hyp, ld_hyp, W, V, pad, eos, tok_logp, score,
                       length, finished);
  else
    hipLaunchKernelGGL(k_hyp_score<false>, dim3(R), dim3(SCORE_THREADS), 0, st, logits, hyp, ld_hyp, W, V, pad, eos, tok_logp, score,
                       length, finished);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

extern "C" int ttx_hypothesis_logprobs(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad,
                                       int eos, float* d_tok_logp, float* d_score, int32_t* d_length, uint8_t* d_finished,
                                       void* stream) {
  if (!s) return session_required("ttx_hypothesis_logprobs");
  if (!d_logits || !d_hyp || !d_score || !d_length) return fail(TTX_ERR_INVALID, "bad argument to ttx_hypothesis_logprobs");
  TTX_TRY(check_score_shapes(s, R, W, V, "ttx_hypothesis_logprobs"));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  return launch_score(s, st, d_logits, d_hyp, W, R, W, V, pad, eos, d_tok_logp, d_score, d_length, d_finished);
}

// The teacher-forced pass of ttx_score_hypotheses / ttx_score_alternatives: the encoder once per source, the full-prefix decoder
// over the B*N rows (row r attends to memory row r / N); logits [B*N, W-1, V] into d_logits.
static int score_forward(ttx_session* s, hipStream_t st, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N,
                         int W, float* d_logits) {
  const ttx_config& c = s->m->cfg;
  const int R = B * N, T = W - 1, d = c.embedding_dim;
  TTX_TRY(ensure(s->memory, (size_t)B * Ls * d * 4, st));
  TTX_TRY(ensure(s->mem_pad_tmp, (size_t)B * Ls, st));
  TTX_TRY(ensure(s->sc_src_of, (size_t)R * 4, st));
  TTX_TRY(ttx_encode_src(s, d_src, B, Ls, s->memory.as<float>(), (void*)st));
  hipLaunchKernelGGL(k_invert_mask, dim3(cdiv(B * Ls, 256)), dim3(256), 0, st, s->src_valid.as<uint8_t>(),
                     s->mem_pad_tmp.as<uint8_t>(), B * Ls);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_score_src_of, dim3(cdiv(R, 256)), dim3(256), 0, st, s->sc_src_of.as<int>(), R, N);
  HIP_TRY(hipGetLastError());
  // decode_tgt(hyp[:, :W-1]) without a sliced copy: the decoder's int32 tokens are read off the strided rows directly
  TTX_TRY(ensure(s->tok_tgt, (size_t)R * T * 4, st));
  hipLaunchKernelGGL(k_prepare_tokens_2d, dim3(cdiv(R * T, 256)), dim3(256), 0, st, d_hyp, ld_hyp, s->tok_tgt.as<int>(),
                     (uint8_t*)nullptr, R, T, c.pad_token);
  HIP_TRY(hipGetLastError());
  return run_decoder_full(s, st, s->tok_tgt.as<int>(), R, T, s->memory.as<float>(), s->mem_pad_tmp.as<uint8_t>(),
                          s->sc_src_of.as<int>(), B, Ls, d_logits);
}

extern "C" int ttx_score_hypotheses(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N,
                                    int W, int eos, float* d_logits, float* d_tok_logp, float* d_score, int32_t* d_length,
                                    uint8_t* d_finished, void* stream) {
  if (!s) return session_required("ttx_score_hypotheses");
  if (!d_src || !d_hyp || !d_score || !d_length || B <= 0 || N <= 0 || Ls <= 0)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_score_hypotheses");
  if (ld_hyp < W) return fail(TTX_ERR_INVALID, "ttx_score_hypotheses: row stride ld_hyp smaller than W");
  const ttx_config& c = s->m->cfg;
  TTX_TRY(check_score_shapes(s, (long long)B * N, W, c.vocab_size, "ttx_score_hypotheses"));
  if (Ls > c.max_positions) return fail(TTX_ERR_INVALID, "source longer than the positional table");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  const int R = B * N, T = W - 1, V = c.vocab_size;
  if (!d_logits) {
    TTX_TRY(ensure(s->ev_logits, (size_t)R * T * V * sizeof(float), st));
    d_logits = s->ev_logits.as<float>();
  }
  TTX_TRY(score_forward(s, st, d_src, B, Ls, d_hyp, ld_hyp, N, W, d_logits));
  return launch_score(s, st, d_logits, d_hyp, ld_hyp, R, W, V, c.pad_token, eos, d_tok_logp, d_score, d_length, d_finished);
}

// ------------------------------------------------------------------------------------------------
// Length-bucketed scoring of a list of batches: csrc/ttx_score_list.hip.h around score_forward + launch_score.
// The caller's batches, checked, as the device table: sources and rows numbered in list order.  src_batch (optional): source -> batch.
static int sl_table(const ttx_session* s, const ttx_score_batch* h, int nb, const int64_t* h_tok_off, const char* fn,
                    std::vector<SlBatch>& tab, int* S_out, int* R_out, std::vector<int>* src_batch) {
  if (!h || nb < 1) return fail(TTX_ERR_INVALID, std::string(fn) + ": an empty list of batches");
  if (s->m->cfg.vocab_size > MET_MAX_V) return fail(TTX_ERR_INVALID, std::string(fn) + ": vocabulary larger than 1024");
  long long S = 0, R = 0;
  tab.resize(nb);
  for (int i = 0; i < nb; ++i) {
    const ttx_score_batch& b = h[i];
    if (!b.d_src || !b.d_hyp || b.B < 1 || b.N < 1 || b.Ls < 1)
      return fail(TTX_ERR_INVALID, std::string(fn) + ": batch " + std::to_string(i) + " needs d_src, d_hyp, B >= 1, N >= 1, Ls >= 1");
    if (b.W < 2) return fail(TTX_ERR_INVALID, std::string(fn) + ": batch " + std::to_string(i) + " has W < 2");
    if (b.ld_hyp < b.W) return fail(TTX_ERR_INVALID, std::string(fn) + ": batch " + std::to_string(i) + " has row stride ld_hyp smaller than W");
    SlBatch& t = tab[i];
    t.src = b.d_src; t.hyp = b.d_hyp; t.B = b.B; t.Ls = b.Ls; t.N = b.N; t.W = b.W; t.ld_hyp = b.ld_hyp;
    t.src0 = (int)S; t.row0 = (int)R; t.pad_ = 0; t.tok0 = h_tok_off ? (long long)h_tok_off[i] : 0;
    if (h_tok_off && h_tok_off[i] < 0) return fail(TTX_ERR_INVALID, std::string(fn) + ": negative tok_logp offset");
    S += b.B;
    R += (long long)b.B * b.N;
    if (R >= (1LL << 31) - 64) return fail(TTX_ERR_INVALID, std::string(fn) + ": more than 2^31 hypothesis rows in one list");
    if (src_batch) src_batch->insert(src_batch->end(), (size_t)b.B, i);
  }
  *S_out = (int)S;
  *R_out = (int)R;
  return TTX_OK;
}

// the table, and `n_extra` int32 words behind it (the run order / a chunk's sources), into sl_tab by ONE stream-ordered copy
static int sl_upload(ttx_session* s, hipStream_t st, const std::vector<SlBatch>& tab, const int32_t* extra, int n_extra,
                     const SlBatch** d_tab, const int** d_extra) {
  const size_t tb = tab.size() * sizeof(SlBatch), bytes = tb + (size_t)n_extra * 4;
  std::vector<char> blob(bytes);
  std::memcpy(blob.data(), tab.data(), tb);
  if (n_extra) std::memcpy(blob.data() + tb, extra, (size_t)n_extra * 4);
  TTX_TRY(ensure(s->sl_tab, bytes, st));
  HIP_TRY(hipMemcpyAsync(s->sl_tab.p, blob.data(), bytes, hipMemcpyHostToDevice, st));   // pageable source: staged before the call returns
  *d_tab = s->sl_tab.as<SlBatch>();
  *d_extra = reinterpret_cast<const int*>(s->sl_tab.as<char>() + tb);
  return TTX_OK;
}

static int sl_launch_extents(ttx_session* s, hipStream_t st, const SlBatch* d_tab, int nb, int S, int R, int eos, int32_t* d_e,
                             int32_t* d_ls, int32_t* d_n, int32_t* d_bad) {
  const ttx_config& c = s->m->cfg;
  HIP_TRY(hipMemsetAsync(d_e, 0, (size_t)S * 4, st));
  if (d_bad) HIP_TRY(hipMemsetAsync(d_bad, 0, 4, st));
  hipLaunchKernelGGL(k_sl_extents, dim3(cdiv(R + S, 4)), dim3(256), 0, st, d_tab, nb, S, R, c.src_vocab_size, c.vocab_size, c.pad_token,
                     eos, d_e, d_ls, d_n, d_bad);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

extern "C" int ttx_score_list_extents(ttx_session* s, const ttx_score_batch* h_batches, int n_batches, int eos, int32_t* d_e,
                                      int32_t* d_ls, int32_t* d_n, int32_t* d_bad, void* stream) {
  if (!s) return session_required("ttx_score_list_extents");
  if (!d_e || !d_ls) return fail(TTX_ERR_INVALID, "bad argument to ttx_score_list_extents: d_e and d_ls are required");
  std::vector<SlBatch> tab;
  int S = 0, R = 0;
  TTX_TRY(sl_table(s, h_batches, n_batches, nullptr, "ttx_score_list_extents", tab, &S, &R, nullptr));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  const SlBatch* d_tab;
  const int* d_none;
  TTX_TRY(sl_upload(s, st, tab, nullptr, 0, &d_tab, &d_none));
  return sl_launch_extents(s, st, d_tab, n_batches, S, R, eos, d_e, d_ls, d_n, d_bad);
}

static int sl_check_chunk(const ttx_session* s, const ttx_score_chunk& ch, const char* fn) {
  const ttx_config& c = s->m->cfg;
  if (ch.count < 1 || ch.N < 1) return fail(TTX_ERR_INVALID, std::string(fn) + ": a chunk needs count >= 1 and N >= 1");
  if (ch.W < 2 || ch.Ls < 1) return fail(TTX_ERR_INVALID, std::string(fn) + ": a chunk needs W >= 2 and Ls >= 1");
  if ((long long)ch.count * ch.N * (ch.W - 1) >= (1LL << 24)) return fail(TTX_ERR_INVALID, std::string(fn) + ": more than 2^24 positions in one chunk");
  if (ch.W - 1 > c.max_positions || ch.Ls > c.max_positions) return fail(TTX_ERR_INVALID, std::string(fn) + ": a chunk wider than the positional table");
  return TTX_OK;
}

static void sl_launch_pack(hipStream_t st, const SlBatch* d_tab, int nb, const int* d_sel, int Bc, int N, int Wc, int Lsc, int pad,
                           int64_t* src_c, int64_t* hyp_c) {
  hipLaunchKernelGGL(k_sl_pack, dim3(cdiv(Bc + Bc * N, 4)), dim3(256), 0, st, d_tab, nb, d_sel, Bc, N, Wc, Lsc, pad, src_c, hyp_c);
}

static void sl_launch_unpack(hipStream_t st, const SlBatch* d_tab, int nb, const int* d_sel, int Bc, int N, int Wc, const float* score_c,
                             const int32_t* length_c, const uint8_t* fin_c, const float* tok_c, float* score, int32_t* length,
                             uint8_t* finished, float* tok) {
  hipLaunchKernelGGL(k_sl_unpack, dim3(cdiv(Bc * N, 4)), dim3(256), 0, st, d_tab, nb, d_sel, Bc, N, Wc, score_c, length_c, fin_c, tok_c,
                     score, length, finished, tok);
}

extern "C" int ttx_score_list_run(ttx_session* s, const ttx_score_batch* h_batches, int n_batches, const int32_t* h_order, int n_order,
                                  const ttx_score_chunk* h_chunks, int n_chunks, int eos, float* d_score, int32_t* d_length,
                                  uint8_t* d_finished, float* d_tok_logp, const int64_t* h_tok_off, void* stream) {
  const char* fn = "ttx_score_list_run";
  if (!s) return session_required(fn);
  if (!h_order || !h_chunks || !d_score || !d_length || n_chunks < 1)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_score_list_run: h_order, h_chunks, d_score and d_length are required");
  if (d_tok_logp && !h_tok_off) return fail(TTX_ERR_INVALID, "ttx_score_list_run: d_tok_logp needs h_tok_off");
  std::vector<SlBatch> tab;
  std::vector<int> src_batch;
  int S = 0, Rtot = 0;
  TTX_TRY(sl_table(s, h_batches, n_batches, d_tok_logp ? h_tok_off : nullptr, fn, tab, &S, &Rtot, &src_batch));
  if (n_order != S) return fail(TTX_ERR_INVALID, "ttx_score_list_run: the order must name every source of the list exactly once");
  std::vector<char> seen((size_t)S, 0);
  long long covered = 0;
  for (int ci = 0; ci < n_chunks; ++ci) {
    const ttx_score_chunk& ch = h_chunks[ci];
    TTX_TRY(sl_check_chunk(s, ch, fn));
    if (ch.first < 0 || (long long)ch.first + ch.count > n_order) return fail(TTX_ERR_INVALID, "ttx_score_list_run: a chunk reaches outside the order");
    for (int j = ch.first; j < ch.first + ch.count; ++j) {
      const int src = h_order[j];
      if (src < 0 || src >= S) return fail(TTX_ERR_INVALID, "ttx_score_list_run: a source index outside the list");
      if (seen[src]) return fail(TTX_ERR_INVALID, "ttx_score_list_run: a source is covered twice");
      seen[src] = 1;
      if (tab[src_batch[src]].N != ch.N) return fail(TTX_ERR_INVALID, "ttx_score_list_run: a chunk holds a source whose batch has another N");
    }
    covered += ch.count;
  }
  if (covered != S) return fail(TTX_ERR_INVALID, "ttx_score_list_run: a source is left out of every chunk");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  const ttx_config& c = s->m->cfg;
  const int V = c.vocab_size;
  const SlBatch* d_tab;
  const int* d_order;
  TTX_TRY(sl_upload(s, st, tab, h_order, n_order, &d_tab, &d_order));
  for (int ci = 0; ci < n_chunks; ++ci) {
    const ttx_score_chunk& ch = h_chunks[ci];
    const int Bc = ch.count, N = ch.N, Wc = ch.W, Lsc = ch.Ls, R = Bc * N, T = Wc - 1;
    const size_t r4 = ((size_t)R * 4 + 15) & ~(size_t)15;
    TTX_TRY(ensure(s->sl_src, (size_t)Bc * Lsc * 8, st));
    TTX_TRY(ensure(s->sl_hyp, (size_t)R * Wc * 8, st));
    TTX_TRY(ensure(s->sl_res, 2 * r4 + (size_t)R, st));
    TTX_TRY(ensure(s->ev_logits, (size_t)R * T * V * sizeof(float), st));
    TTX_TRY(ensure(s->ev_nll, (size_t)R * T * sizeof(float), st));
    float* score_c = s->sl_res.as<float>();
    int32_t* length_c = reinterpret_cast<int32_t*>(s->sl_res.as<char>() + r4);
    uint8_t* fin_c = reinterpret_cast<uint8_t*>(s->sl_res.as<char>() + 2 * r4);
    const int* d_sel = d_order + ch.first;
    sl_launch_pack(st, d_tab, n_batches, d_sel, Bc, N, Wc, Lsc, c.pad_token, s->sl_src.as<int64_t>(), s->sl_hyp.as<int64_t>());
    HIP_TRY(hipGetLastError());
    // what ttx_score_hypotheses runs, on the packed rows
    TTX_TRY(score_forward(s, st, s->sl_src.as<int64_t>(), Bc, Lsc, s->sl_hyp.as<int64_t>(), Wc, N, Wc, s->ev_logits.as<float>()));
    TTX_TRY(launch_score(s, st, s->ev_logits.as<float>(), s->sl_hyp.as<int64_t>(), Wc, R, Wc, V, c.pad_token, eos, s->ev_nll.as<float>(),
                         score_c, length_c, fin_c));
    sl_launch_unpack(st, d_tab, n_batches, d_sel, Bc, N, Wc, score_c, length_c, fin_c, s->ev_nll.as<float>(), d_score, d_length,
                     d_finished, d_tok_logp);
    HIP_TRY(hipGetLastError());
  }
  return TTX_OK;
}

extern "C" int ttx_debug_score_list(ttx_session* s, int op, const ttx_score_batch* h_batches, int n_batches, const int32_t* h_sel,
                                    int n_sel, const int64_t* h_tok_off, const ttx_debug_score_list_args* a, void* stream) {
  const char* fn = "ttx_debug_score_list";
  if (!s) return session_required(fn);
  if (!a || op < 0 || op > 2) return fail(TTX_ERR_INVALID, "bad argument to ttx_debug_score_list: op 0, 1 or 2 and its operands");
  std::vector<SlBatch> tab;
  std::vector<int> src_batch;
  int S = 0, R = 0;
  TTX_TRY(sl_table(s, h_batches, n_batches, (op == 2 && a->d_tok_logp) ? h_tok_off : nullptr, fn, tab, &S, &R, &src_batch));
  if (op == 0) {
    if (!a->d_e || !a->d_ls) return fail(TTX_ERR_INVALID, "ttx_debug_score_list: op 0 needs d_e and d_ls");
  } else {
    if (!h_sel || n_sel < 1) return fail(TTX_ERR_INVALID, "ttx_debug_score_list: ops 1 and 2 need the chunk's sources");
    TTX_TRY(sl_check_chunk(s, ttx_score_chunk{0, n_sel, a->N, a->W, a->Ls < 1 && op == 2 ? 1 : a->Ls}, fn));
    for (int j = 0; j < n_sel; ++j)
      if (h_sel[j] < 0 || h_sel[j] >= S || tab[src_batch[h_sel[j]]].N != a->N)
        return fail(TTX_ERR_INVALID, "ttx_debug_score_list: a source outside the list or of a batch with another N");
    if (op == 1 && (!a->d_src_c || !a->d_hyp_c)) return fail(TTX_ERR_INVALID, "ttx_debug_score_list: op 1 needs d_src_c and d_hyp_c");
    if (op == 2 && (!a->d_score_c || !a->d_length_c || !a->d_fin_c || !a->d_score || !a->d_length))
      return fail(TTX_ERR_INVALID, "ttx_debug_score_list: op 2 needs the chunk's score, length and finished and d_score, d_length");
    if (op == 2 && a->d_tok_logp && (!a->d_tok_c || !h_tok_off)) return fail(TTX_ERR_INVALID, "ttx_debug_score_list: d_tok_logp needs d_tok_c and h_tok_off");
  }
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  const SlBatch* d_tab;
  const int* d_sel;
  TTX_TRY(sl_upload(s, st, tab, h_sel, op == 0 ? 0 : n_sel, &d_tab, &d_sel));
  if (op == 0) return sl_launch_extents(s, st, d_tab, n_batches, S, R, a->eos, a->d_e, a->d_ls, a->d_n, a->d_bad);
  if (op == 1)
    sl_launch_pack(st, d_tab, n_batches, d_sel, n_sel, a->N, a->W, a->Ls, s->m->cfg.pad_token, a->d_src_c, a->d_hyp_c);
  else
    sl_launch_unpack(st, d_tab, n_batches, d_sel, n_sel, a->N, a->W, a->d_score_c, a->d_length_c, a->d_fin_c, a->d_tok_c, a->d_score,
                     a->d_length, a->d_finished, a->d_tok_logp);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Folding hypotheses into their distinct ones: csrc/ttx_fold.hip.h.  One launch, no workspace: the session only names the device.
extern "C" int ttx_fold_hypotheses(ttx_session* s, const int64_t* d_hyp, int B, int N, int W, int ld_hyp, int pad, int eos,
                                   const float* d_score, int order, int flags, int32_t* d_first, int32_t* d_rank_of,
                                   int32_t* d_n_unique, int32_t* d_perm, int32_t* d_count, float* d_out_score, int64_t* d_out,
                                   float* d_logmass, void* stream) {
  if (!d_hyp || B < 1 || N < 1 || W < 1) return fail(TTX_ERR_INVALID, "bad argument to ttx_fold_hypotheses: d_hyp, B >= 1, N >= 1, W >= 1");
  if (N > FOLD_MAX_N) return fail(TTX_ERR_INVALID, "ttx_fold_hypotheses: more than 1024 rows per source");
  if (ld_hyp < W) return fail(TTX_ERR_INVALID, "ttx_fold_hypotheses: row stride ld_hyp smaller than W");
  if (order != TTX_FOLD_FIRST && order != TTX_FOLD_SCORE && order != TTX_FOLD_COUNT)
    return fail(TTX_ERR_INVALID, "ttx_fold_hypotheses: unknown order");
  if (flags & ~(TTX_FOLD_UNFINISHED_LAST | TTX_FOLD_DEBUG_NO_FILTER)) return fail(TTX_ERR_INVALID, "ttx_fold_hypotheses: unknown flag bit");
  if (!d_score && order == TTX_FOLD_SCORE) return fail(TTX_ERR_INVALID, "ttx_fold_hypotheses: the SCORE order needs scores");
  if (!d_score && d_logmass) return fail(TTX_ERR_INVALID, "ttx_fold_hypotheses: logmass needs scores");
  if (!d_first && !d_rank_of && !d_n_unique && !d_perm && !d_count && !d_out_score && !d_out && !d_logmass)
    return fail(TTX_ERR_INVALID, "ttx_fold_hypotheses: no output requested");
  if (s) {
    HIP_TRY(hipSetDevice(s->m->device));
  } else {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
      return fail(TTX_ERR_NO_DEVICE, "no HIP device visible; libttx_hip has no CPU fallback");
  }
  hipStream_t st = (hipStream_t)stream;
  FoldArgs a{};
  a.hyp = d_hyp; a.score_in = d_score; a.first = d_first; a.rank_of = d_rank_of; a.n_unique = d_n_unique; a.perm = d_perm;
  a.count = d_count; a.score = d_out_score; a.out = d_out; a.logmass = d_logmass;
  a.N = N; a.W = W; a.ld_hyp = ld_hyp; a.pad = pad; a.eos = eos; a.order = order; a.flags = flags;
  // 16-byte row copies: every source and destination row starts on 16 bytes (W and ld_hyp even, both bases aligned)
  const bool vec2 = d_out && W % 2 == 0 && ld_hyp % 2 == 0 && reinterpret_cast<uintptr_t>(d_hyp) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
  if (vec2)
    hipLaunchKernelGGL(k_fold_hyps<true>, dim3(B), dim3(FOLD_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL(k_fold_hyps<false>, dim3(B), dim3(FOLD_THREADS), 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Per-position alternatives of hypotheses: csrc/ttx_alternatives.hip.h.
static int check_alt_args(int V, int k, const void* top_id, const void* top_logp, const void* chosen, const void* rank,
                          const void* entropy, const char* fn) {
  if (k < 1) return fail(TTX_ERR_INVALID, std::string(fn) + ": k must be at least 1");
  if (k > ALT_MAX_K) return fail(TTX_ERR_INVALID, std::string(fn) + ": k larger than 32");
  if (k > V) return fail(TTX_ERR_INVALID, std::string(fn) + ": k larger than the vocabulary");
  if (!top_id && !top_logp && !chosen && !rank && !entropy)
    return fail(TTX_ERR_INVALID, std::string(fn) + ": no output requested (top_id, top_logp, chosen_logp, rank and entropy are all null)");
  return TTX_OK;
}

// k_hyp_length, then ONE launch of k_alternatives over all R*T positions.  The column order follows V alone; the 16-byte loads
// are chosen from the base address and give the same bits as the 4-byte ones.
static int launch_alternatives(ttx_session* s, hipStream_t st, const float* logits, const int64_t* hyp, int ld_hyp, int R, int W, int V,
                               int pad, int eos, int k, int32_t* top_id, float* top_logp, float* chosen, int32_t* rank, float* entropy,
                               int32_t* length) {
  if (!length) {
    TTX_TRY(ensure(s->am_length, (size_t)R * 4, st));
    length = s->am_length.as<int32_t>();
  }
  hipLaunchKernelGGL(k_hyp_length, dim3(cdiv(R, 4)), dim3(256), 0, st, hyp, ld_hyp, R, W, pad, eos, length);
  HIP_TRY(hipGetLastError());
  AltArgs a{};
  a.logits = logits; a.hyp = hyp; a.length = length; a.top_id = top_id; a.top_logp = top_logp; a.chosen_logp = chosen;
  a.rank = rank; a.entropy = entropy; a.ld_hyp = ld_hyp; a.M = R * (W - 1); a.T = W - 1; a.V = V; a.k = k;
  const dim3 grid(cdiv(a.M, 4)), block(256);
  if (V % 4 != 0) hipLaunchKernelGGL((k_alternatives<false, false>), grid, block, 0, st, a);
  else if (reinterpret_cast<uintptr_t>(logits) % 16 == 0) hipLaunchKernelGGL((k_alternatives<true, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((k_alternatives<true, false>), grid, block, 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

extern "C" int ttx_hypothesis_alternatives(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad,
                                           int eos, int k, int32_t* d_top_id, float* d_top_logp, float* d_chosen_logp,
                                           int32_t* d_rank, float* d_entropy, int32_t* d_length, void* stream) {
  if (!s) return session_required("ttx_hypothesis_alternatives");
  if (!d_logits || !d_hyp) return fail(TTX_ERR_INVALID, "bad argument to ttx_hypothesis_alternatives");
  TTX_TRY(check_score_shapes(s, R, W, V, "ttx_hypothesis_alternatives"));
  TTX_TRY(check_alt_args(V, k, d_top_id, d_top_logp, d_chosen_logp, d_rank, d_entropy, "ttx_hypothesis_alternatives"));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  return launch_alternatives(s, st, d_logits, d_hyp, W, R, W, V, pad, eos, k, d_top_id, d_top_logp, d_chosen_logp, d_rank, d_entropy,
                             d_length);
}

extern "C" int ttx_score_alternatives(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N,
                                      int W, int eos, int k, float* d_logits, int32_t* d_top_id, float* d_top_logp,
                                      float* d_chosen_logp, int32_t* d_rank, float* d_entropy, int32_t* d_length, void* stream) {
  if (!s) return session_required("ttx_score_alternatives");
  if (!d_src || !d_hyp || B <= 0 || N <= 0 || Ls <= 0) return fail(TTX_ERR_INVALID, "bad argument to ttx_score_alternatives");
  if (ld_hyp < W) return fail(TTX_ERR_INVALID, "ttx_score_alternatives: row stride ld_hyp smaller than W");
  const ttx_config& c = s->m->cfg;
  TTX_TRY(check_score_shapes(s, (long long)B * N, W, c.vocab_size, "ttx_score_alternatives"));
  TTX_TRY(check_alt_args(c.vocab_size, k, d_top_id, d_top_logp, d_chosen_logp, d_rank, d_entropy, "ttx_score_alternatives"));
  if (Ls > c.max_positions) return fail(TTX_ERR_INVALID, "source longer than the positional table");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  const int R = B * N, T = W - 1, V = c.vocab_size;
  if (!d_logits) {
    TTX_TRY(ensure(s->ev_logits, (size_t)R * T * V * sizeof(float), st));
    d_logits = s->ev_logits.as<float>();
  }
  TTX_TRY(score_forward(s, st, d_src, B, Ls, d_hyp, ld_hyp, N, W, d_logits));
  return launch_alternatives(s, st, d_logits, d_hyp, ld_hyp, R, W, V, c.pad_token, eos, k, d_top_id, d_top_logp, d_chosen_logp, d_rank,
                             d_entropy, d_length);
}

// ------------------------------------------------------------------------------------------------
// A kernel whose dynamic LDS exceeds the default limit has the limit raised once per session (`done`), outside graph capture.
static int raise_lds_limit(const void* kernel, size_t lds, bool& done) {
  if (lds > 64 * 1024 && !done) {
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    done = true;
  }
  return TTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Cross-attention maps of hypotheses: csrc/ttx_attn_probs.hip.h.
static int attn_probs_key_limit(int head_dim) { return (head_dim == 32 || head_dim == 64) ? AP_MAX_KEYS : 0; }

template <int DH>
static int launch_attn_probs_dh(ttx_session* s, hipStream_t st, const AttnProbsArgs& a, bool vec_out, bool vec_k, size_t lds) {
  const int grid = a.R * cdiv(a.T, AP_TQ);
  bool* done = &s->attr_attn_probs[(DH == 64 ? 4 : 0) + (vec_out ? 2 : 0) + (vec_k ? 1 : 0)];
#define TTX_AP_LAUNCH(VO, VK)                                                                                        \
  do {                                                                                                               \
    TTX_TRY(raise_lds_limit(reinterpret_cast<const void*>(&k_attn_probs<DH, VO, VK>), lds, *done));                  \
    hipLaunchKernelGGL((k_attn_probs<DH, VO, VK>), dim3(grid), dim3(AP_THREADS), lds, st, a);                        \
  } while (0)
  if (vec_out && vec_k) TTX_AP_LAUNCH(true, true);
  else if (vec_out) TTX_AP_LAUNCH(true, false);
  else if (vec_k) TTX_AP_LAUNCH(false, true);
  else TTX_AP_LAUNCH(false, false);
#undef TTX_AP_LAUNCH
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// ONE launch of k_attn_probs.  The 16-byte forms are chosen from the arguments alone and give the same bits as the 4-byte ones.
static int launch_attn_probs(ttx_session* s, hipStream_t st, const AttnProbsArgs& a, int head_dim) {
  const int limit = attn_probs_key_limit(head_dim);
  if (limit == 0) return fail(TTX_ERR_INVALID, "attention maps: head dimension must be 32 or 64");
  if (a.R <= 0 || a.Rm <= 0 || a.H <= 0 || a.T <= 0 || a.Ls <= 0 || a.ldq < a.H * head_dim || a.ldkv < a.H * head_dim)
    return fail(TTX_ERR_INVALID, "attention maps: R, Rm, H, T, Ls > 0 and ldq, ldkv >= H * head_dim");
  if (a.Ls > limit)
    return fail(TTX_ERR_INVALID, "attention maps: source longer than " + std::to_string(limit) + " keys (ttx_attn_probs_key_limit)");
  if ((long long)a.R * a.T >= (1LL << 24)) return fail(TTX_ERR_INVALID, "attention maps: more than 2^24 positions in one call");
  auto al16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  const bool vec_out = a.Ls % 4 == 0 && al16(a.heads) && al16(a.mean);
  const bool vec_k = a.ldkv % 4 == 0 && al16(a.k);
  const size_t lds = ap_lds_bytes(a.Ls, head_dim, a.mean || a.align);
  return head_dim == 64 ? launch_attn_probs_dh<64>(s, st, a, vec_out, vec_k, lds) : launch_attn_probs_dh<32>(s, st, a, vec_out, vec_k, lds);
}

extern "C" int ttx_attn_probs_key_limit(int head_dim) { return attn_probs_key_limit(head_dim); }

extern "C" int ttx_debug_attn_probs(ttx_session* s, const float* d_q, int ldq, const float* d_k, int ldkv, const uint8_t* d_key_pad,
                                    const int32_t* d_mem_row, const int32_t* d_length, int R, int Rm, int H, int head_dim, int T,
                                    int Ls, float scale, float* d_heads, float* d_mean, int32_t* d_align, void* stream) {
  if (!s) return session_required("ttx_debug_attn_probs");
  if (!d_q || !d_k || !d_key_pad || !d_length || (!d_heads && !d_mean && !d_align))
    return fail(TTX_ERR_INVALID, "bad argument to ttx_debug_attn_probs");
  if (!d_mem_row && Rm != R) return fail(TTX_ERR_INVALID, "ttx_debug_attn_probs: without a row map the memory must have one row per query row");
  HIP_TRY(hipSetDevice(s->m->device));
  AttnProbsArgs a{};
  a.q = d_q; a.ldq = ldq; a.k = d_k; a.ldkv = ldkv; a.key_pad = d_key_pad; a.mem_row = d_mem_row; a.length = d_length;
  a.heads = d_heads; a.mean = d_mean; a.align = d_align; a.R = R; a.Rm = Rm; a.H = H; a.T = T; a.Ls = Ls; a.scale = scale;
  return launch_attn_probs(s, reinterpret_cast<hipStream_t>(stream), a, head_dim);
}

extern "C" int ttx_attention_maps(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W,
                                  int eos, int layer, float* d_heads, float* d_mean, int32_t* d_align, int32_t* d_length,
                                  void* stream) {
  if (!s) return session_required("ttx_attention_maps");
  if (!d_src || !d_hyp || B <= 0 || N <= 0 || Ls <= 0) return fail(TTX_ERR_INVALID, "bad argument to ttx_attention_maps");
  if (!d_heads && !d_mean && !d_align) return fail(TTX_ERR_INVALID, "ttx_attention_maps: no output requested (heads, mean and alignment are all null)");
  if (ld_hyp < W) return fail(TTX_ERR_INVALID, "ttx_attention_maps: row stride ld_hyp smaller than W");
  const ttx_config& c = s->m->cfg;
  if (layer == -1) layer = c.num_decoder_layers - 1;
  if (layer < 0 || layer >= c.num_decoder_layers)
    return fail(TTX_ERR_INVALID, "ttx_attention_maps: layer must be -1 or in [0, " + std::to_string(c.num_decoder_layers) + ")");
  // the position limits of scoring; its vocabulary limit does not apply (no logits are formed)
  TTX_TRY(check_score_shapes(s, (long long)B * N, W, 1, "ttx_attention_maps"));
  if (Ls > c.max_positions) return fail(TTX_ERR_INVALID, "source longer than the positional table");
  const int limit = attn_probs_key_limit(c.embedding_dim / c.num_heads);
  if (Ls > limit)
    return fail(TTX_ERR_INVALID, "ttx_attention_maps: source longer than " + std::to_string(limit) + " keys (ttx_attn_probs_key_limit)");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  const int R = B * N, T = W - 1, d = c.embedding_dim;
  if (!d_length) {
    TTX_TRY(ensure(s->am_length, (size_t)R * 4, st));
    d_length = s->am_length.as<int32_t>();
  }
  // as ttx_score_hypotheses: the encoder once per source; decoder row r attends to memory row r / N
  TTX_TRY(ensure(s->memory, (size_t)B * Ls * d * 4, st));
  TTX_TRY(ensure(s->mem_pad_tmp, (size_t)B * Ls, st));
  TTX_TRY(ensure(s->sc_src_of, (size_t)R * 4, st));
  TTX_TRY(ttx_encode_src(s, d_src, B, Ls, s->memory.as<float>(), stream));
  hipLaunchKernelGGL(k_invert_mask, dim3(cdiv(B * Ls, 256)), dim3(256), 0, st, s->src_valid.as<uint8_t>(),
                     s->mem_pad_tmp.as<uint8_t>(), B * Ls);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_score_src_of, dim3(cdiv(R, 256)), dim3(256), 0, st, s->sc_src_of.as<int>(), R, N);
  HIP_TRY(hipGetLastError());
  TTX_TRY(ensure(s->tok_tgt, (size_t)R * T * 4, st));
  hipLaunchKernelGGL(k_prepare_tokens_2d, dim3(cdiv(R * T, 256)), dim3(256), 0, st, d_hyp, ld_hyp, s->tok_tgt.as<int>(),
                     (uint8_t*)nullptr, R, T, c.pad_token);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_hyp_length, dim3(cdiv(R, 4)), dim3(256), 0, st, d_hyp, ld_hyp, R, W, c.pad_token, eos, d_length);
  HIP_TRY(hipGetLastError());
  const AttnTap tap{layer, d_length, d_heads, d_mean, d_align};
  return run_decoder_full(s, st, s->tok_tgt.as<int>(), R, T, s->memory.as<float>(), s->mem_pad_tmp.as<uint8_t>(),
                          s->sc_src_of.as<int>(), B, Ls, nullptr, &tap);
}

static int clamp_draft_len(int draft_len, int lo, int hi) { return std::min(std::max(lo, draft_len), hi); }

template <typename OutT>
static int launch_make_drafts(hipStream_t st, const int* src32, int src_ld, int off, int B, int L, int N, int D, int eos,
                              int pad, int repl, OutT* out) {
  const int need = N + D - 1;
  const int Lp = L > need ? L : need;
  const size_t lds = sizeof(int) * (size_t)(Lp + 1);
  if (lds > 60 * 1024) return fail(TTX_ERR_INVALID, "make_drafts: padded source row too long");
  hipLaunchKernelGGL((k_make_drafts<OutT>), dim3(B), dim3(64), lds, st, src32, src_ld, off, L, N, D, eos, pad, repl, out);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

extern "C" int ttx_make_drafts(ttx_session* s, const int64_t* d_src, int B, int L, int draft_len, int n_drafts,
                               int min_draft_len, int max_draft_len, int eos_token, int pad_token, int replace_token,
                               int64_t* d_drafts, void* stream) {
  if (!s || !d_src || !d_drafts || B <= 0 || L <= 0) return fail(TTX_ERR_INVALID, "bad argument to ttx_make_drafts");
  // the reference's assertions (drafting.py:39-43)
  if (n_drafts <= 0) return fail(TTX_ERR_REFERENCE, "The number of drafts must be greater than 0");
  if (min_draft_len > max_draft_len) return fail(TTX_ERR_REFERENCE, "The minimum draft length must not be greater than the maximum draft length");
  if (pad_token == replace_token || eos_token == replace_token || eos_token == pad_token)
    return fail(TTX_ERR_REFERENCE, "pad, eos and replace tokens must be pairwise different");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  const int D = clamp_draft_len(draft_len, min_draft_len, max_draft_len);
  if (D <= 0) return fail(TTX_ERR_INVALID, "draft length must be positive");
  TTX_TRY(ensure(s->src32, (size_t)B * L * 4, st));
  TTX_TRY(prepare_tokens(st, d_src, s->src32.as<int>(), nullptr, B * L, pad_token));
  return launch_make_drafts<int64_t>(st, s->src32.as<int>(), L, 0, B, L, n_drafts, D, eos_token, pad_token, replace_token, d_drafts);
}

// ------------------------------------------------------------------------------------------------
// One verify step of the greedy-speculative loop: D+1 new positions per (running row, draft) through the
// decoder with the KV cache, argmax, accept/retire, K/V commit.  Every kernel sizes its work from the
// device-resident DecState, so the launch sequence is identical for every step (graph-replayable).
struct StepCtx {
  int B, Ls, N, D, Lc, gen_ld, max_len;
  ttx_gen_params p;
  const float* kcache = nullptr;   // null: the session's greedy-path caches
  const float* vcache = nullptr;
  const int* src_of = nullptr;     // running row -> source row (tree decoding)
  const int* src_len = nullptr;    // slot pool: source keys per slot
  const int* cache_slot = nullptr; // batch pool: running row (candidate) -> slot of its KV cache
  bool want_argmax = true;
  bool want_sample = false;        // sampling loop: k_sample on `sample` where k_argmax would run
  SampleArgs sample{};
  bool want_sample_step = false;   // speculative sampling loop: k_sample_step on `sample`'s key, sample and prm
  const int* pfx_draft0 = nullptr; // prompted or proposed speculative sampling (sample.pfx or prop set): the rows' source draft 0, [B, D]
  PrefixTab prop{};                // proposed speculative sampling: the proposals, offered as draft 0 and never forced (sample.pfx unset)
  int prop_ctx = PROPOSAL_CTX;     // context tokens k_proposal_drafts compares per shift
  int variant = GV_BIG;           // GemmVariant of this step's launches (bit-identical results; chosen from the live row count)
  // two-phase verify step of the slot pool; unset (null): the session's state, active list, step QKV buffer and argmax buffer
  DecState* st_ov = nullptr;       // live rows of this pass
  const int* act_ov = nullptr;     // sequences of this pass
  float* qkv_ov = nullptr;         // [Ld][B * RPS][3d]
  int* pred_ov = nullptr;          // [B * RPS]
  int sel_N = 0, sel_D = 0;        // probe: the layout of the draft pass, whose choice between k_attn2 and k_attn it takes
  // draft select (draft pass of a split step; all null otherwise): the pass's rows are stored compacted (k_probe_split)
  const int* row_base = nullptr; const int* draft_mask = nullptr; const int* row_map = nullptr;
  // per-source logit bias (val null: none, no launch): k_logit_bias between the classifier and the consumer of the logits.  `src` goes
  // by decoder row (slot of a pool; candidate of a beam loop); the values live in a session buffer, never in the caller's tensor
  LogitBiasTab bias{};
  // syntax constraint (null: none, no launch): k_syntax_mask after the bias and before the consumer.  The class table lives in a session
  // buffer; the rule's max_len and EOS are the step's (max_len, p.eos_token), the state comes from gen / drafts
  const signed char* syntax = nullptr;
};

// k_syntax_mask with k_logit_bias's launch shape, in place on `a.logits`; `step`: the step-row layout.
static int launch_syntax_mask(hipStream_t st, const SyntaxArgs& a, bool step) {
  const dim3 grid(cdiv(a.M, 4)), block(256);
  if (step) hipLaunchKernelGGL((k_syntax_mask<true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((k_syntax_mask<false>), grid, block, 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// k_logit_bias with k_sample's launch shape, in place on `a.logits`; `step`: the step-row layout (act_idx, row_map, N, D set).
static int launch_logit_bias(hipStream_t st, const LogitBiasArgs& a, bool step) {
  const dim3 grid(cdiv(a.M, 4)), block(256);
  if (step) hipLaunchKernelGGL((k_logit_bias<true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((k_logit_bias<false>), grid, block, 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// k_sample with k_argmax's launch shape; the values a lane holds follow the vocabulary (V <= SAMPLE_MAX_V, checked by the callers).
static int launch_sample(hipStream_t st, const SampleArgs& a) {
  const dim3 grid(cdiv(a.M, 4)), block(256);
  if (a.V <= 64) hipLaunchKernelGGL((k_sample<1>), grid, block, 0, st, a);
  else if (a.V <= 128) hipLaunchKernelGGL((k_sample<2>), grid, block, 0, st, a);
  else if (a.V <= 256) hipLaunchKernelGGL((k_sample<4>), grid, block, 0, st, a);
  else if (a.V <= 512) hipLaunchKernelGGL((k_sample<8>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((k_sample<16>), grid, block, 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// k_sample_step with the same launch shape and the same choice of VPL.
static int launch_sample_step(hipStream_t st, const SampleStepArgs& a) {
  const dim3 grid(cdiv(a.M, 4)), block(256);
  if (a.V <= 64) hipLaunchKernelGGL((k_sample_step<1>), grid, block, 0, st, a);
  else if (a.V <= 128) hipLaunchKernelGGL((k_sample_step<2>), grid, block, 0, st, a);
  else if (a.V <= 256) hipLaunchKernelGGL((k_sample_step<4>), grid, block, 0, st, a);
  else if (a.V <= 512) hipLaunchKernelGGL((k_sample_step<8>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((k_sample_step<16>), grid, block, 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// k_prefix_drafts on the session's loop state: draft 0 of every active row, one wave per slot, grid for the capacity.
static int launch_prefix_drafts_args(hipStream_t st, const PrefixDraftsArgs& a, int B) {
  hipLaunchKernelGGL(k_prefix_drafts, dim3(cdiv(B, 4)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// k_proposal_drafts with k_prefix_drafts' launch shape.
static int launch_proposal_drafts_args(hipStream_t st, const ProposalDraftsArgs& a, int B) {
  hipLaunchKernelGGL(k_proposal_drafts, dim3(cdiv(B, 4)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// The table a prompted or a proposed call carries through pool admission (a call is one or the other), tok null for neither.
static const PrefixTab& step_tab(const StepCtx& k) { return k.sample.pfx.tok ? k.sample.pfx : k.prop; }

// The head of every verify step of a prompted or a proposed speculative sampling loop; nothing for any other loop.
static int launch_prefix_drafts(ttx_session* s, hipStream_t st, const StepCtx& k) {
  if (k.prop.tok && k.want_sample_step) {
    ProposalDraftsArgs a{};
    a.st = s->state.as<DecState>(); a.act_idx = s->act_idx.as<int>(); a.front = s->front.as<int>();
    a.gen = s->gen.as<int>(); a.gen_ld = k.gen_ld;
    a.drafts = s->drafts.as<int>(); a.N = k.N; a.D = k.D; a.draft0 = k.pfx_draft0; a.tab = k.prop;
    a.bos = k.p.bos_token; a.eos = k.p.eos_token; a.pad = k.p.pad_token; a.repl = k.p.replace_token; a.ctx = k.prop_ctx;
    return launch_proposal_drafts_args(st, a, k.B);
  }
  if (!k.sample.pfx.tok || !k.want_sample_step) return TTX_OK;
  PrefixDraftsArgs a{};
  a.st = s->state.as<DecState>(); a.act_idx = s->act_idx.as<int>(); a.front = s->front.as<int>();
  a.drafts = s->drafts.as<int>(); a.N = k.N; a.D = k.D; a.draft0 = k.pfx_draft0; a.pfx = k.sample.pfx;
  a.eos = k.p.eos_token; a.pad = k.p.pad_token; a.repl = k.p.replace_token;
  return launch_prefix_drafts_args(st, a, k.B);
}

static int run_step(ttx_session* s, hipStream_t st, const StepCtx& k, int kcap) {
  const ttx_model* m = s->m;
  const ttx_config& c = m->cfg;
  const int d = c.embedding_dim, H = c.num_heads, V = c.vocab_size, Ld = c.num_decoder_layers;
  const int D1 = k.D + 1;
  const int RPS = step_rps(k.N, k.D);
  const int Mmax = k.B * RPS;
  DecState* dst = k.st_ov ? k.st_ov : s->state.as<DecState>();
  const int* act = k.act_ov ? k.act_ov : s->act_idx.as<int>();
  const int* m_ptr = &dst->m_rows;
  float* ao = s->ao.as<float>();
  float* logits = s->logits.as<float>();
  const float scale = 1.0f / sqrtf((float)(d / H));
  const long long cache_seq = (long long)k.Lc * d;
  const long long cache_layer = (long long)k.B * cache_seq;

  struct AttnSel {                 // the attention launches of this step choose their kernel as the layout (sel_N, sel_D) does
    ttx_session* s;
    AttnSel(ttx_session* s_, int N, int D) : s(s_) { s->attn_sel_N = N; s->attn_sel_D = D; }
    ~AttnSel() { s->attn_sel_N = 0; s->attn_sel_D = 0; }
  } attn_sel(s, k.sel_N, k.sel_D);
  EmbedArgs e{};
  e.table = m->p(m->tgt_emb); e.pe = m->p(m->pe); e.X = s->x.as<float>(); e.d = d; e.V = c.vocab_size;
  e.st = dst; e.act_idx = act; e.front = s->front.as<int>(); e.gen = s->gen.as<int>(); e.gen_ld = k.gen_ld;
  e.drafts = s->drafts.as<int>(); e.N = k.N; e.D = k.D; e.row_map = k.row_map;
  hipLaunchKernelGGL((k_embed<true>), dim3(cdiv(Mmax, 4)), dim3(256), 0, st, e);
  HIP_TRY(hipGetLastError());

  const StackRows rows{m_ptr, Mmax, variant_qkv(k.variant), variant_dd(k.variant), variant_ffn1(k.variant), variant_ffn2(k.variant),
                       k.qkv_ov ? k.qkv_ov : s->qkv.as<float>(), (long long)Mmax * 3 * d};
  TTX_TRY(run_decoder_stack(s, st, rows,
      [&](int l, float* qkv) -> int {
        AttnArgs a{};
        a.q = qkv; a.ldq = 3 * d; a.k = qkv + d; a.v = qkv + 2 * d; a.ldkv = 3 * d; a.out = ao; a.d = d; a.scale = scale;
        a.tok = s->gen.as<int>(); a.pad = c.pad_token; a.st = dst; a.act_idx = act; a.front = s->front.as<int>();
        a.kcache = (k.kcache ? k.kcache : s->kcache.as<float>()) + (size_t)l * cache_layer;
        a.vcache = (k.vcache ? k.vcache : s->vcache.as<float>()) + (size_t)l * cache_layer;
        a.cache_seq_stride = cache_seq; a.gen_ld = k.gen_ld; a.N = k.N; a.D = k.D; a.cache_slot = k.cache_slot;
        a.row_base = k.row_base; a.draft_mask = k.draft_mask;
        return launch_attn(ATT_STEP_SELF, s, st, a, k.B, H, RPS, kcap, k.N, D1);
      },
      [&](int l) -> int {
        AttnArgs ca{};
        ca.q = s->q2.as<float>(); ca.ldq = d; ca.k = s->memkv.as<float>() + (size_t)l * 2 * d; ca.v = ca.k + d; ca.ldkv = Ld * 2 * d;
        ca.out = ao; ca.d = d; ca.scale = scale; ca.Lk = k.Ls; ca.key_pad = s->src_valid.as<uint8_t>();
        ca.st = dst; ca.act_idx = act; ca.front = s->front.as<int>(); ca.N = k.N; ca.D = k.D;
        ca.src_of = k.src_of; ca.src_len = k.src_len; ca.row_base = k.row_base; ca.draft_mask = k.draft_mask;
        return launch_attn(ATT_STEP_CROSS, s, st, ca, k.B, H, RPS, k.Ls, k.N, D1);
      },
      logits));
  if (k.bias.val) {                  // one launch, and none in an unbiased step
    LogitBiasArgs b{};
    b.logits = logits; b.V = V; b.m_ptr = m_ptr; b.M = Mmax; b.tab = k.bias; b.rows_per_src = 1;
    if (!k.want_sample) { b.act_idx = act; b.row_map = k.row_map; b.N = k.N; b.D = k.D; }
    TTX_TRY(launch_logit_bias(st, b, !k.want_sample));
    s->logit_bias_launches += 1;
  }
  if (k.syntax) {                    // after the bias (-inf stays -inf), before the consumer; none in an unconstrained step
    SyntaxArgs y{};
    y.logits = logits; y.V = V; y.m_ptr = m_ptr; y.M = Mmax; y.cls = k.syntax; y.max_len = k.max_len; y.eos = k.p.eos_token;
    y.gen = s->gen.as<int>(); y.gen_ld = k.gen_ld; y.front = s->front.as<int>();
    if (!k.want_sample) { y.act_idx = act; y.row_map = k.row_map; y.drafts = s->drafts.as<int>(); y.N = k.N; y.D = k.D; }
    TTX_TRY(launch_syntax_mask(st, y, !k.want_sample));
    s->syntax_launches += 1;
  }
  if (k.want_sample) {
    SampleArgs a = k.sample;
    a.logits = logits; a.V = V; a.pred = s->pred.as<int>(); a.m_ptr = m_ptr; a.M = Mmax;
    return launch_sample(st, a);
  }
  if (k.want_sample_step) {
    SampleStepArgs a{};
    a.logits = logits; a.V = V; a.pred = k.pred_ov ? k.pred_ov : s->pred.as<int>(); a.m_ptr = m_ptr; a.M = Mmax;
    a.key = k.sample.key; a.sample = k.sample.sample; a.prm = k.sample.prm;
    a.act_idx = act; a.front = s->front.as<int>(); a.N = k.N; a.D = k.D; a.row_map = k.row_map; a.pfx = k.sample.pfx;
    return launch_sample_step(st, a);
  }
  if (k.want_argmax) {
    hipLaunchKernelGGL(k_argmax, dim3(cdiv(Mmax, 4)), dim3(256), 0, st, logits, V, k.pred_ov ? k.pred_ov : s->pred.as<int>(), m_ptr, Mmax);
    HIP_TRY(hipGetLastError());
  }
  return TTX_OK;
}

struct GenCtx {
  StepCtx k;
  LoopArgs la;
  KvCopyArgs kc;
};

// The accept step of a speculative loop over B slots: k_accept alone, or with `la.blk` set (accept_blk_for) the pair.
static int launch_accept(hipStream_t st, const LoopArgs& la, int threads) {
  if (la.blk) {
    hipLaunchKernelGGL(k_accept_slots, dim3(cdiv(la.B, ACCEPT_SLOT_WAVES)), dim3(ACCEPT_SLOT_WAVES * 64), 0, st, la);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_accept_finish, dim3(1), dim3(ACCEPT_THREADS), 0, st, la);
  } else {
    hipLaunchKernelGGL(k_accept, dim3(1), dim3(threads ? threads : (la.B > 256 ? ACCEPT_THREADS : 256)), 0, st, la);
  }
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// The accept step of the speculative sampling loop: one workgroup with k_accept's block size, or with `la.blk` set (the sampling
// pool above 256 slots, accept_blk_for) the pair k_sample_accept_slots, k_accept_finish.
static int launch_sample_accept(hipStream_t st, const LoopArgs& la) {
  if (la.blk) {
    hipLaunchKernelGGL(k_sample_accept_slots, dim3(cdiv(la.B, ACCEPT_SLOT_WAVES)), dim3(ACCEPT_SLOT_WAVES * 64), 0, st, la);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_accept_finish, dim3(1), dim3(ACCEPT_THREADS), 0, st, la);
  } else {
    hipLaunchKernelGGL(k_sample_accept, dim3(1), dim3(la.B > 256 ? ACCEPT_THREADS : 256), 0, st, la);
  }
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// The session's AcceptBlk for loops of more than 256 slots (null otherwise, and with TTX_ACCEPT_SPREAD=0): zero when fresh, and
// left zero by every k_accept_finish.  The choice follows the capacity alone, as k_accept's block size does.
// `spread`: the switch as the caller reads it (the session's TTX_ACCEPT_SPREAD, or the sampling pool's reading at pool start).
static int accept_blk_when(ttx_session* s, hipStream_t st, int B, bool spread, AcceptBlk** out) {
  *out = nullptr;
  if (!spread || B <= 256) return TTX_OK;
  const void* before = s->accept_blk.p;
  TTX_TRY(ensure(s->accept_blk, sizeof(AcceptBlk), st));
  if (s->accept_blk.p != before) HIP_TRY(hipMemsetAsync(s->accept_blk.p, 0, sizeof(AcceptBlk), st));
  *out = s->accept_blk.as<AcceptBlk>();
  return TTX_OK;
}
static int accept_blk_for(ttx_session* s, hipStream_t st, int B, AcceptBlk** out) { return accept_blk_when(s, st, B, s->accept_spread, out); }

static int launch_accept_and_commit(ttx_session* s, hipStream_t st, const GenCtx& g, bool greedy) {
  if (greedy) {
    hipLaunchKernelGGL(k_greedy_accept, dim3(1), dim3(256), 0, st, g.la);
    HIP_TRY(hipGetLastError());
  } else if (g.la.sample_rule) {
    TTX_TRY(launch_sample_accept(st, g.la));
  } else {
    TTX_TRY(launch_accept(st, g.la, 0));
  }
  hipLaunchKernelGGL(k_kvcopy, dim3(g.k.B, s->m->cfg.num_decoder_layers), dim3(256), 0, st, g.kc);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// A verify step did not publish within the watchdog time.  The stream may be stuck for good, so NOTHING here (or in the
// callers, on this path) synchronises it: the session is marked unusable, every later call on it fails at once, and
// destroying it leaks its workspaces instead of waiting for the device.  The process should report the error and exit
// non-zero (or continue in a fresh child process); it must not re-exec itself after having touched the GPU.
static int session_hung(ttx_session* s) {
  s->dead = true;
  return fail(TTX_ERR_HIP, "verify step did not publish its result within the watchdog time; the session is unusable "
                           "(its stream was NOT synchronised) - exit the process or continue in a fresh child process");
}

static int session_alive(const ttx_session* s) {
  if (s && s->dead) return fail(TTX_ERR_HIP, "this session hung in an earlier call and is unusable");
  return TTX_OK;
}

// Key capacity of a step whose rows see fewer than `width` prefix keys: the LDS images of the self-attention come in buckets of
// 64 keys, so that a graph serves 64 widths.
static int key_capacity(int width, int max_len) { return std::min(max_len, ((width + 63) / 64) * 64); }

// Enqueue the launch sequence `enqueue()` puts on `st`: eagerly when graphs are off (TTX_NO_GRAPH, profiling sessions) and the
// first time `key` is seen (function attributes, i.e. dynamic LDS limits, are set outside capture); captured into `cache` the
// second time; replayed from the captured graph from then on.
template <class Enqueue>
static int graph_replay(ttx_session* s, hipStream_t st, GraphCache& cache, const GraphKey& key, Enqueue&& enqueue) {
  if (!s->use_graphs || s->profile) return enqueue();
  const auto now = [s] { return s->host_timing ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point(); };
  const auto us_since = [&](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::micro>(now() - t0).count(); };
  s->graphs_current();                             // captured pointers may be stale
  auto it = cache.map.find(key);
  if (it == cache.map.end()) {
    if (cache.warmed.insert(key).second) return enqueue();
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    const auto t0 = now();
    HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    hipError_t e = hipStreamEndCapture(st, &graph);
    if (rc != TTX_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(TTX_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(TTX_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    if (cache.map.size() > cache.limit) s->drop_graphs();
    it = cache.map.emplace(key, exec).first;
    if (s->host_timing) { s->host_captures += 1; s->host_capture_us += us_since(t0); }
  }
  const auto t0 = now();
  HIP_TRY(hipGraphLaunch(it->second, st));
  if (s->host_timing) { s->host_launches += 1; s->host_launch_us += us_since(t0); }
  return TTX_OK;
}

// LoopArgs and KvCopyArgs of a speculative loop over the g.k.B slots of the session's greedy-path buffers: everything but the output
// buffer and the per-row trace (gen_start) and the pool's own fields (pool_start), which the caller sets after the call.
static int fill_loop_args(ttx_session* s, GenCtx& g, AcceptBlk* blk) {
  const StepCtx& k = g.k;
  const int d = s->m->cfg.embedding_dim;
  LoopArgs& la = g.la;
  la.st = s->state.as<DecState>(); la.act_idx = s->act_idx.as<int>(); la.front = s->front.as<int>();
  la.gen = s->gen.as<int>(); la.gen_ld = k.gen_ld; la.drafts = s->drafts.as<int>(); la.pred = s->pred.as<int>();
  la.rec = s->rec.as<CopyRec>(); la.haspad = s->haspad.as<int>();
  HIP_TRY(hipHostGetDevicePointer((void**)&la.host, (void*)s->host_info, 0));
  la.B = k.B; la.N = k.N; la.D = k.D; la.Ls = k.Ls; la.max_len = k.max_len; la.pad = k.p.pad_token; la.bos = k.p.bos_token;
  la.eos = k.p.eos_token; la.traj_ld = k.max_len + 1; la.blk = blk;
  KvCopyArgs& kc = g.kc;
  kc.st = la.st; kc.rec = la.rec; kc.qkv = s->qkv.as<float>();
  kc.qkv_layer_stride = (long long)k.B * step_rps(k.N, k.D) * 3 * d;
  kc.kcache = s->kcache.as<float>(); kc.vcache = s->vcache.as<float>();
  kc.cache_seq_stride = (long long)k.Lc * d; kc.cache_layer_stride = (long long)k.B * k.Lc * d;
  kc.N = k.N; kc.D = k.D; kc.d = d;
  return TTX_OK;
}

struct EventGuard {              // destroys the event on every exit path
  hipEvent_t e = nullptr;
  ~EventGuard() { if (e) (void)hipEventDestroy(e); }
};

// One call decoding on sessions[0 .. n) from this host thread, each session on its own stream (the caller's may be the legacy null
// stream, which cannot be captured into a graph).  Every session stream first waits for what the caller's stream holds; then
// start(i) runs for each session in turn, and drive_jobs (ttx_drive.h) hands out turn(i) until every session has finished.
// Whatever ends the call, a stream that was given work has drained when it returns, so the caller may free its buffers and
// sees the outputs from whatever it enqueues next.  The one exception is a hang: nothing is synchronised then, every session
// of the call is retired, and the call returns what session_hung set.
template <class Start, class TurnFn>
static int drive_sessions(ttx_session** sessions, int n, bool serial, void* stream, Start&& start, TurnFn&& turn) {
  for (int i = 0; i < n; ++i) TTX_TRY(session_alive(sessions[i]));
  HIP_TRY(hipSetDevice(sessions[0]->m->device));
  release_retired();
  EventGuard ready;
  HIP_TRY(hipEventCreateWithFlags(&ready.e, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(ready.e, (hipStream_t)stream));
  const auto after_caller = [&](ttx_session* s) -> int {
    TTX_TRY(ensure_own_stream(s));
    HIP_TRY(hipStreamWaitEvent(s->own_stream, ready.e, 0));
    return TTX_OK;
  };
  DriveResult r{TTX_OK, false, -1};
  int given = 0;                   // sessions whose stream may hold work of this call
  while (given < n && r.rc == TTX_OK) {
    r.rc = after_caller(sessions[given]);
    if (r.rc == TTX_OK) r.rc = start(given);
    ++given;
  }
  if (r.rc == TTX_OK) r = drive_jobs(n, serial, watchdog_seconds(), turn);
  if (r.hung) {
    // a stream that never published may never drain: do not wait on any of them, and retire every session of this call
    // (their workspaces may still be written by whatever is stuck)
    const int rc = session_hung(sessions[r.stalled_job]);
    for (int i = 0; i < n; ++i) sessions[i]->dead = true;
    return rc;
  }
  for (int i = 0; i < given; ++i)
    if (sessions[i]->own_stream) (void)hipStreamSynchronize(sessions[i]->own_stream);
  return r.rc;
}

// One generate call in flight on one session: start (encoder, drafts, loop init) -> steps -> finish.
struct GenJob {
  ttx_session* s = nullptr;
  hipStream_t st = nullptr;
  GenCtx g{};
  bool greedy = false;
  int64_t* d_out = nullptr;
  int16_t* d_traj = nullptr;     // per-row rule only: [B][max_len + 1] fronts after every step (-1 past the row's last step)
  int32_t* d_fin = nullptr;      // per-row rule only: [B] step at which the row produced EOS (0: never)
  ttx_gen_stats* stats = nullptr;
  int launched = 0;
  int phase = 0;          // 0 idle, 1 running, 2 finishing
  int batch = -1;
};

static int gen_validate(const ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_gen_params* p, const int64_t* d_out,
                        bool greedy) {
  if (!s || !d_src || !p || !d_out || B <= 0 || Ls <= 1) return fail(TTX_ERR_INVALID, "bad argument to a generate call");
  const ttx_config& c = s->m->cfg;
  if (!greedy) {
    if (p->n_drafts <= 0) return fail(TTX_ERR_REFERENCE, "The number of drafts must be greater than 0");
    if (p->max_len < 1) return fail(TTX_ERR_REFERENCE, "The minimum draft length must not be greater than the maximum draft length");
    if (p->pad_token == p->replace_token || p->eos_token == p->replace_token || p->eos_token == p->pad_token)
      return fail(TTX_ERR_REFERENCE, "pad, eos and replace tokens must be pairwise different");
    if (p->draft_len <= 0) return fail(TTX_ERR_REFERENCE, "Number of speculative tokens must be a positive integer.");
    if (p->draft_len > p->max_len) return fail(TTX_ERR_REFERENCE, "draft_len beyond max_len: the reference's scatter shapes disagree");
  } else if (p->max_len < 1) {
    return fail(TTX_ERR_INVALID, "max_len must be positive");
  }
  if (p->pad_token != c.pad_token) return fail(TTX_ERR_INVALID, "generator pad token differs from the model's");
  const int D = greedy ? 0 : p->draft_len;
  if (p->max_len + D + 2 > c.max_positions) return fail(TTX_ERR_INVALID, "max_len + draft_len exceeds the positional table");
  return TTX_OK;
}

// `per_src` > 1 (sampling loop): the B decoder rows are per_src consecutive rows per source, d_src holds B / per_src sources, and
// the caller sets StepCtx::src_of before the first step.  `sample_rule` (speculative sampling): the copy drafts of a source are made
// once and replicated to its per_src decoder rows (k_embed and the accept step keep indexing drafts by decoder row), and the loop
// runs under LoopArgs::sample_rule.
static int gen_start(GenJob& j, ttx_session* s, hipStream_t st, const int64_t* d_src, int B, int Ls, const ttx_gen_params* p,
                     int64_t* d_out, ttx_gen_stats* stats, bool greedy, int16_t* d_traj, int32_t* d_fin, int per_src,
                     bool sample_rule) {
  const int d = s->m->cfg.embedding_dim, Ld = s->m->cfg.num_decoder_layers;
  const int N = greedy ? 1 : p->n_drafts, D = greedy ? 0 : p->draft_len, D1 = D + 1;
  const int max_len = p->max_len;
  j.s = s; j.st = st; j.greedy = greedy; j.d_out = d_out; j.stats = stats; j.launched = 0;
  j.d_traj = d_traj; j.d_fin = d_fin;
  const bool row_rule = d_traj != nullptr;
  s->snap_step = 0;
  GenCtx& g = j.g;
  g = GenCtx{};
  g.k.B = B; g.k.Ls = Ls; g.k.N = N; g.k.D = D; g.k.max_len = max_len; g.k.p = *p;
  g.k.Lc = max_len + D1;           // cache positions per row (front + D < max_len + D)
  g.k.gen_ld = max_len + D + 2;
  const size_t Mmax = (size_t)B * step_rps(N, D);
  const int Bs = B / per_src;      // sources

  Needs need{st};
  need(s->tok_src, (size_t)Bs * Ls * 4); need(s->src_valid, (size_t)Bs * Ls); need(s->memory, (size_t)Bs * Ls * d * 4);
  need(s->memkv, (size_t)Bs * Ls * Ld * 2 * d * 4);
  need(s->drafts, (size_t)B * N * std::max(D, 1) * 4);
  need(s->gen, (size_t)B * g.k.gen_ld * 4); need(s->front, (size_t)B * 4); need(s->act_idx, (size_t)B * 4); need(s->haspad, (size_t)B * 4);
  if (row_rule) { need(s->traj, (size_t)B * (max_len + 1) * 2); need(s->fin_step, (size_t)B * 4); }
  need(s->rec, (size_t)B * sizeof(CopyRec)); need(s->outbuf, (size_t)B * max_len * 8);
  need(s->kcache, (size_t)Ld * B * g.k.Lc * d * 4); need(s->vcache, (size_t)Ld * B * g.k.Lc * d * 4);
  need_step_workspaces(s, need, Mmax, (size_t)Bs * Ls);
  TTX_TRY(need.rc);
  AcceptBlk* blk = nullptr;
  if (!greedy && !sample_rule) TTX_TRY(accept_blk_for(s, st, B, &blk));
  if (!greedy && per_src > 1) TTX_TRY(ensure(s->smp_drafts, (size_t)Bs * N * D * 4, st));
  s->graphs_current();                                            // captured pointers may be stale

  s->ev_used = 0;
  HIP_TRY(hipEventRecord(s->ev_a, st));
  // encoder once per batch (:60-61) + cross-attention K/V of every decoder layer once per source
  TTX_TRY(encode_sources(s, st, d_src, 0, Bs, Ls, s->src_valid.as<uint8_t>(), s->memkv.as<float>()));
  // drafts from src[:, 1:] (:64-73): min_draft_len 1, max_draft_len max_len
  if (!greedy) {
    TTX_TRY(launch_make_drafts<int>(st, s->tok_src.as<int>(), Ls, 1, Bs, Ls - 1, N, D, p->eos_token, p->pad_token,
                                    p->replace_token, per_src > 1 ? s->smp_drafts.as<int>() : s->drafts.as<int>()));
    if (per_src > 1) {
      hipLaunchKernelGGL(k_sample_rep_drafts, dim3(cdiv(B * N * D, 256)), dim3(256), 0, st, s->smp_drafts.as<int>(), s->drafts.as<int>(),
                         B, per_src, N * D);
      HIP_TRY(hipGetLastError());
    }
  }

  TTX_TRY(fill_loop_args(s, g, blk));
  g.la.out = s->outbuf.as<int64_t>();
  g.la.sample_rule = sample_rule ? 1 : 0;
  g.la.row_rule = row_rule ? 1 : 0; g.la.traj = row_rule ? s->traj.as<short>() : nullptr;
  g.la.fin_step = row_rule ? s->fin_step.as<int>() : nullptr;

  s->host_info->stop = 0;
  s->host_info->steps_done = 0;
  s->host_info->width = 1;
  s->host_info->n_active = B;
  hipLaunchKernelGGL(k_loop_init, dim3(64), dim3(256), 0, st, g.la);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev_b, st));
  j.phase = 1;
  return TTX_OK;
}

// Enqueue one verify step through graph_replay, one graph per (shape, key-capacity bucket); the step whose logits the caller
// asked for (want_logits) runs eagerly.  `width_bound` bounds the reference's generated width when the step runs.
static int gen_launch_step(GenJob& j, int width_bound) {
  ttx_session* s = j.s;
  StepCtx k = j.g.k;
  // GEMM variant from the rows this step will have (published by the previous step's accept kernel; plain greedy decoding
  // keeps all B rows): a free choice, every variant returns the same bits
  const int live = j.greedy ? k.B : std::max(1, (int)((volatile HostInfo*)s->host_info)->n_active);
  k.variant = variant_for_rows(s, (long long)live * step_rps(k.N, k.D), true);
  const int kcap = key_capacity(std::max(width_bound, 1), k.max_len);        // prefix keys this step can see: < width_bound
  const auto enqueue = [&]() -> int {
    TTX_TRY(launch_prefix_drafts(s, j.st, k));
    TTX_TRY(run_step(s, j.st, k, kcap));
    return launch_accept_and_commit(s, j.st, j.g, j.greedy);
  };
  if (k.p.want_logits > 0 && k.p.want_logits == j.launched + 1) {
    // the snapshot step runs eagerly: keep its pre-argmax logits and the loop state they belong to (before accept changes it)
    TTX_TRY(launch_prefix_drafts(s, j.st, k));       // the head of a prompted step, as in `enqueue` (the sampling calls ask for no snapshot today)
    TTX_TRY(run_step(s, j.st, k, kcap));
    const ttx_config& c = s->m->cfg;
    const size_t Mmax = (size_t)k.B * step_rps(k.N, k.D);
    TTX_TRY(ensure(s->snap_logits, Mmax * c.vocab_size * 4, j.st));
    TTX_TRY(ensure(s->snap_act, (size_t)k.B * 4, j.st));
    TTX_TRY(ensure(s->snap_front, (size_t)k.B * 4, j.st));
    TTX_TRY(ensure(s->snap_gen, (size_t)k.B * k.gen_ld * 4, j.st));
    TTX_TRY(ensure(s->snap_state, sizeof(DecState), j.st));
    HIP_TRY(hipMemcpyAsync(s->snap_logits.p, s->logits.p, Mmax * c.vocab_size * 4, hipMemcpyDeviceToDevice, j.st));
    HIP_TRY(hipMemcpyAsync(s->snap_act.p, s->act_idx.p, (size_t)k.B * 4, hipMemcpyDeviceToDevice, j.st));
    HIP_TRY(hipMemcpyAsync(s->snap_front.p, s->front.p, (size_t)k.B * 4, hipMemcpyDeviceToDevice, j.st));
    HIP_TRY(hipMemcpyAsync(s->snap_gen.p, s->gen.p, (size_t)k.B * k.gen_ld * 4, hipMemcpyDeviceToDevice, j.st));
    HIP_TRY(hipMemcpyAsync(s->snap_state.p, s->state.p, sizeof(DecState), hipMemcpyDeviceToDevice, j.st));
    s->snap_B = k.B; s->snap_rps = step_rps(k.N, k.D); s->snap_gen_ld = k.gen_ld; s->snap_step = j.launched + 1;
    TTX_TRY(launch_accept_and_commit(s, j.st, j.g, j.greedy));
  } else {
    const bool pfx = k.sample.pfx.tok != nullptr;  // a prompted call never shares a graph with an unprompted one
    const bool prop = k.prop.tok != nullptr;       // nor does a proposed one; its keys end with the context length of the launch
    const int site = k.want_sample_step ? (prop ? GS_STEP_SAMPLE_SPEC_PROPOSAL : pfx ? GS_STEP_SAMPLE_SPEC_PREFIX : GS_STEP_SAMPLE_SPEC)
                     : k.want_sample    ? (pfx ? GS_STEP_SAMPLE_PREFIX : GS_STEP_SAMPLE)
                     : j.greedy ? GS_STEP_GREEDY : (j.g.la.row_rule ? GS_STEP_ROW_RULE : GS_STEP_SPECULATIVE);
    GraphKey key{site | (k.bias.val ? GS_LOGIT_BIAS : 0) | (k.syntax ? GS_SYNTAX : 0), k.B, k.Ls, k.N, k.D, k.max_len, kcap, k.variant, 0};
    if (prop) key.push_back(k.prop_ctx);
    TTX_TRY(graph_replay(s, j.st, s->step_graphs, key, enqueue));
  }
  ++j.launched;
  return TTX_OK;
}

// The last thing a job enqueues: the end of the decode phase (ev_c), the `bytes` counters at `d_counters` into the pinned
// host_state, and ev_done, which the job's turn polls before it reads them.
static int enqueue_readback(ttx_session* s, hipStream_t st, const void* d_counters, size_t bytes) {
  HIP_TRY(hipEventRecord(s->ev_c, st));
  HIP_TRY(hipMemcpyAsync(s->host_state, d_counters, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(s->ev_done, st));
  return TTX_OK;
}

// The counters a finished job read back, added to `st` (a single batch starts from zeroes).
static void add_counters(ttx_gen_stats& st, const DecState& hs) {
  st.model_calls += hs.steps;
  st.accepted_tokens += hs.accepted;
  st.produced_tokens += hs.produced;
  st.verified_positions += hs.verified_positions;
  st.kv_prefix_positions += hs.kv_prefix_positions;
  st.src_positions += hs.src_positions;
}

static void add_counters(ttx_beam_stats& st, const BeamCounters& cn) {
  st.model_calls += cn.model_calls;
  st.input_lines += cn.input_lines;
  st.running_rows += cn.running_rows;
  st.verified_positions += cn.verified_positions;
  st.executed_positions += cn.executed_positions;
  st.kv_prefix_positions += cn.kv_prefix_positions;
  st.running_candidates += cn.running_cands;
}

static int gen_finish_enqueue(GenJob& j) {
  ttx_session* s = j.s;
  const StepCtx& k = j.g.k;
  if (j.greedy) {
    hipLaunchKernelGGL(k_gen_to_out, dim3(cdiv(k.B * k.max_len, 256)), dim3(256), 0, j.st, s->gen.as<int>(), k.gen_ld, j.d_out,
                       k.B, k.max_len);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemcpyAsync(j.d_out, s->outbuf.as<int64_t>(), (size_t)k.B * k.max_len * 8, hipMemcpyDeviceToDevice, j.st));
    if (j.d_traj) {
      HIP_TRY(hipMemcpyAsync(j.d_traj, s->traj.p, (size_t)k.B * (k.max_len + 1) * 2, hipMemcpyDeviceToDevice, j.st));
      HIP_TRY(hipMemcpyAsync(j.d_fin, s->fin_step.p, (size_t)k.B * 4, hipMemcpyDeviceToDevice, j.st));
    }
  }
  TTX_TRY(enqueue_readback(s, j.st, s->state.p, sizeof(DecState)));
  j.phase = 2;
  return TTX_OK;
}

// GEMM event pairs of the work just finished on `st` -> the session's running sums (bench.py roofline).
static void collect_gemm_profile(ttx_session* s, hipStream_t st) {
  if (!s->profile) return;
  // summed over the generate calls since the last ttx_last_kernel_profile read
  s->prof_launches += (long long)s->ev_used;
  for (size_t i = 0; i < s->ev_used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->ev_pool[i].first, s->ev_pool[i].second) == hipSuccess) s->prof_ms += ms;
  }
  s->ev_used = 0;
  // What the bracketing itself adds to a launch's figure: pairs around a kernel of known duration (k_spin reports the
  // realtime ticks it saw go by), pair time minus in-kernel time, median of 32.
  if (s->prof_empty_pair_ms < 0 && s->ev_pool.size() >= 32) {
    unsigned long long* d_ticks = nullptr;
    if (hipMalloc(&d_ticks, 32 * sizeof(unsigned long long)) == hipSuccess) {
      for (int i = 0; i < 32; ++i) {
        (void)hipEventRecord(s->ev_pool[i].first, st);
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st, d_ticks + i, 2000);          // 20 us
        (void)hipEventRecord(s->ev_pool[i].second, st);
      }
      (void)hipStreamSynchronize(st);
      unsigned long long h_ticks[32];
      std::vector<double> over;
      if (hipMemcpy(h_ticks, d_ticks, sizeof(h_ticks), hipMemcpyDeviceToHost) == hipSuccess)
        for (int i = 0; i < 32; ++i) {
          float ms = 0.f;
          if (hipEventElapsedTime(&ms, s->ev_pool[i].first, s->ev_pool[i].second) == hipSuccess)
            over.push_back((double)ms - (double)h_ticks[i] * 1e-5);                        // 100 MHz ticks -> ms
        }
      (void)hipFree(d_ticks);
      if (!over.empty()) {
        std::sort(over.begin(), over.end());
        s->prof_empty_pair_ms = std::max(0.0, over[over.size() / 2]);
      }
    }
  }
}

// What the finishing turns of the three pools share: the pool's device time (ev_a to ev_c) added to *decode_ms, and the GEMM event
// pairs.  collect_gemm_profile reads and re-records the ev_pool pairs alone, never ev_a or ev_c, so the order of the two is free.
static void pool_finish(ttx_session* s, hipStream_t st, double* decode_ms) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, s->ev_a, s->ev_c) == hipSuccess) *decode_ms += ms;
  collect_gemm_profile(s, st);
}

static int gen_finish_collect(GenJob& j) {
  ttx_session* s = j.s;
  const DecState& hs = *s->host_state;
  if (j.stats) {
    *j.stats = ttx_gen_stats{};
    add_counters(*j.stats, hs);
    j.stats->src_tokens_padded = (long long)j.g.k.B * j.g.k.Ls;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev_a, s->ev_b));
    j.stats->encode_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev_b, s->ev_c));
    j.stats->decode_ms = ms;
  }
  collect_gemm_profile(s, j.st);
  j.phase = 0;
  if (j.stats) j.stats->status = hs.error == 3 ? TTX_ERR_ROW_REPLAY : (hs.error ? TTX_ERR_REFERENCE : TTX_OK);
  if (hs.error == 3)
    return fail(TTX_ERR_ROW_REPLAY, "a row emitted PAD inside its sequence: what the reference does next depends on the other rows "
                                    "of its batch, so the batch must be decoded as given (ttx_greedy_speculative_generate_many)");
  if (hs.error == 2)
    return fail(TTX_ERR_REFERENCE, "the model emitted PAD inside a sequence and a whole column became PAD: the reference's draft "
                                   "scatter raises 'index out of range' here (speculative_decoding.py:97,111-115)");
  if (hs.error) return fail(TTX_ERR_REFERENCE, "a row finished at a width beyond max_len: shape mismatch in the reference (speculative_decoding.py:158)");
  return TTX_OK;
}

// The sampling loop's additions to a greedy generate call (ttx_sample_generate): B counts decoder rows, n of them per source; and
// the one host-side record of a call's constraints (constraints_validate fills them; the beam loops read nothing else of it).
struct SampleSetup {
  int n;
  const int64_t* d_row_keys;       // [B / n] or null
  SampleBlock blk;
  bool spec;                       // ttx_sample_speculative_generate: the speculative loop with k_sample_step and k_sample_accept
  // forced prefixes; prompted false: the call is the unprompted one, launch for launch
  bool prompted;
  const int64_t* d_prefix; int ld_prefix; const int32_t* h_prefix_len; int n_sources;
  // proposal drafts: the table rides in the prefix fields above and through the same workspaces, since a call is either prompted
  // or proposed; proposed false: no proposal, launch for launch
  bool proposed; int prop_ctx;
  bool tabled() const { return prompted || proposed; }
  // per-source logit bias: d_bias null is the unbiased call, launch for launch; [n_sources][ld_bias]
  const float* d_bias; int ld_bias;
  // syntax constraint: the caller's class table int8 [V] on the device, null for the unconstrained call
  const signed char* d_syntax;
  bool any() const { return tabled() || d_bias || d_syntax; }
};

// The names a call's refusals carry.  The feature that introduced an argument named its refusals after its own entry point, so a body
// behind several forms keeps up to four: `call` for the loop's parameters, `ex` for prefix, proposal and filter, `bias`, `syntax`.
struct Who {
  const char* call; const char* ex; const char* bias; const char* syntax;
  Who(const char* w) : call(w), ex(w), bias(w), syntax(w) {}
  Who(const char* c, const char* e, const char* b, const char* y) : call(c), ex(e), bias(b), syntax(y) {}
};

// The prefix arguments of a sampling call over S sources, or TTX_ERR_INVALID.  A call whose lengths are all zero (or absent) is
// not prompted: it runs the unprompted call's launches and graphs.
static int prefix_validate(const char* who, const int64_t* d_prefix, int ld_prefix, const int32_t* h_prefix_len, int S, int max_len,
                           SampleSetup* smp) {
  smp->prompted = false; smp->d_prefix = d_prefix; smp->ld_prefix = ld_prefix; smp->h_prefix_len = h_prefix_len; smp->n_sources = S;
  if (!h_prefix_len) return TTX_OK;
  if (ld_prefix < 0) return fail(TTX_ERR_INVALID, std::string(who) + ": ld_prefix must not be negative");
  for (int i = 0; i < S; ++i) {
    const int n = h_prefix_len[i];
    if (n < 0 || n > max_len - 1) return fail(TTX_ERR_INVALID, std::string(who) + ": a prefix length must lie in [0, max_len - 1]");
    if (n > ld_prefix) return fail(TTX_ERR_INVALID, std::string(who) + ": a prefix length exceeds ld_prefix");
    if (n > 0 && !d_prefix) return fail(TTX_ERR_INVALID, std::string(who) + ": a prefix length is non-zero but d_prefix is null");
    smp->prompted |= n > 0;
  }
  return TTX_OK;
}

// The constraints of a call over `n_sources` sources whose rows have `max_len` columns into `smp`, or TTX_ERR_INVALID; nothing of
// `smp` but its constraint fields is touched.  In order: the bias (ld_bias at least the vocabulary; the values are the caller's to
// keep finite or -inf, they live on the device), the syntax table (a null struct or a null table is the unconstrained call; its
// max_len is 0 or the call's), the prefix, and the proposal, which is held to a prefix's limits and refused beside a non-empty prefix.
// A proposed call keeps its table in the prefix fields.  The proposal's context length is PROPOSAL_CTX; TTX_PROPOSAL_CTX (2, 4 or 8,
// read per call) overrides it for measurements and changes no output.  A zeroed `o` and a null `syn` leave `smp` unconstrained.
static int constraints_validate(const Who& who, const ttx_session* s, const ttx_sample_opts& o, const ttx_syntax* syn, int n_sources,
                                int max_len, SampleSetup* smp) {
  if (o.d_bias && o.ld_bias < s->m->cfg.vocab_size) return fail(TTX_ERR_INVALID, std::string(who.bias) + ": ld_bias must be at least the vocabulary");
  smp->d_bias = o.d_bias; smp->ld_bias = o.ld_bias; smp->d_syntax = nullptr;
  if (syn && syn->d_cls) {
    if (syn->max_len != 0 && syn->max_len != max_len)
      return fail(TTX_ERR_INVALID, std::string(who.syntax) + ": ttx_syntax.max_len must be 0 or the call's max_len");
    smp->d_syntax = reinterpret_cast<const signed char*>(syn->d_cls);
  }
  TTX_TRY(prefix_validate(who.ex, o.d_prefix, o.ld_prefix, o.h_prefix_len, n_sources, max_len, smp));
  smp->proposed = false; smp->prop_ctx = PROPOSAL_CTX;
  if (!o.h_proposal_len) return TTX_OK;
  SampleSetup q{};
  const std::string who_q = std::string(who.ex) + " (the proposal, held to a prefix's limits)";
  TTX_TRY(prefix_validate(who_q.c_str(), o.d_proposal, o.ld_proposal, o.h_proposal_len, n_sources, max_len, &q));
  if (!q.prompted) return TTX_OK;
  if (smp->prompted) return fail(TTX_ERR_INVALID, std::string(who.ex) + ": a call takes forced prefixes or proposals, not both");
  smp->d_prefix = o.d_proposal; smp->ld_prefix = o.ld_proposal; smp->h_prefix_len = o.h_proposal_len;
  smp->proposed = true;
  if (const char* e = getenv("TTX_PROPOSAL_CTX")) {
    const int c = atoi(e);
    if (c != 2 && c != 4 && c != 8) return fail(TTX_ERR_INVALID, std::string(who.ex) + ": TTX_PROPOSAL_CTX must be 2, 4 or 8");
    smp->prop_ctx = c;
  }
  return TTX_OK;
}

// The session buffers of a call's constraints, sized before anything is captured and before the loop's start settles which graphs
// are current: the table of prefixes (or proposals) int32 [sources][max_len] with the sources' lengths, `rows` per-row lengths and
// `draft0` saved first-draft tokens (the samplers' rows or slots; 0 where the table goes by source), the bias float [sources][V],
// the class table int8 [V], and `src_of` entries of the row-to-source map smp_src_of (the samplers' rows; the sources of a prompted
// beam loop; 0 for the pools, whose slots keep maps of their own).
static int constraints_ensure(ttx_session* s, hipStream_t st, const SampleSetup& c, int max_len, size_t rows, size_t draft0, size_t src_of) {
  const size_t S = c.n_sources, V = s->m->cfg.vocab_size;
  if (c.tabled()) {
    TTX_TRY(ensure(s->pfx_tok, S * max_len * 4, st));
    TTX_TRY(ensure(s->pfx_len_src, S * 4, st));
    TTX_TRY(ensure(s->pfx_len, rows * 4, st));
    TTX_TRY(ensure(s->pfx_draft0, draft0 * 4, st));
  }
  if (c.d_bias) TTX_TRY(ensure(s->lb_val, S * V * sizeof(float), st));
  if (c.d_syntax) TTX_TRY(ensure(s->syn_cls, V, st));
  return ensure(s->smp_src_of, src_of * 4, st);
}

// What the steps of a constrained loop read, in the session's copies; pfx.tok, bias.val, syntax: null for a call without that one.
struct ConstraintTabs { PrefixTab pfx{}; LogitBiasTab bias{}; const signed char* syntax = nullptr; };

// The caller's bias, class table and prefix (or proposal) table into the session's copies, so that a captured step reads the session's
// buffers and nothing of the call; enqueued outside capture, before the first step.  The row length of the bias is the vocabulary and
// that of the prefix table max_len, which every step key holds.  How a decoder row finds its source differs per loop and is the
// caller's: `pfx_len` and `pfx_src` (the rows' prefix lengths and table rows) and `bias_src`, device arrays the loop fills.
static int constraints_upload(ttx_session* s, hipStream_t st, const SampleSetup& c, int max_len, int pad, const int* pfx_len,
                              const int* pfx_src, const int* bias_src, ConstraintTabs* t) {
  const int S = c.n_sources, V = s->m->cfg.vocab_size;
  *t = ConstraintTabs{};
  if (c.d_bias) {
    HIP_TRY(hipMemcpy2DAsync(s->lb_val.p, (size_t)V * sizeof(float), c.d_bias, (size_t)c.ld_bias * sizeof(float), (size_t)V * sizeof(float),
                             (size_t)S, hipMemcpyDeviceToDevice, st));
    t->bias = LogitBiasTab{s->lb_val.as<float>(), V, bias_src};
  }
  if (c.d_syntax) {
    HIP_TRY(hipMemcpyAsync(s->syn_cls.p, c.d_syntax, (size_t)V, hipMemcpyDeviceToDevice, st));
    t->syntax = s->syn_cls.as<signed char>();
  }
  if (c.tabled()) {
    HIP_TRY(hipMemcpyAsync(s->pfx_len_src.p, c.h_prefix_len, (size_t)S * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_prefix_load, dim3(cdiv(S * max_len, 256)), dim3(256), 0, st, c.d_prefix, c.ld_prefix, s->pfx_len_src.as<int>(),
                       s->pfx_tok.as<int>(), S, max_len, pad);
    HIP_TRY(hipGetLastError());
    t->pfx = PrefixTab{s->pfx_tok.as<int>(), max_len, pfx_len, pfx_src};
  }
  return TTX_OK;
}

// Session buffers of the sampling loop, sized before anything is captured.
static int sample_ensure(ttx_session* s, hipStream_t st, size_t rows, const SampleSetup& smp, const ttx_gen_params* p) {
  TTX_TRY(constraints_ensure(s, st, smp, p->max_len, rows, smp.spec ? rows * p->draft_len : 0, rows));
  TTX_TRY(ensure(s->smp_key, rows * 8, st));
  TTX_TRY(ensure(s->smp_sample, rows * 4, st));
  TTX_TRY(ensure(s->smp_done, rows * 4, st));
  return ensure(s->smp_prm, sizeof(SampleBlock), st);
}

// After gen_start: the rows' keys, sample ids, done flags and sources and the call's parameter block on the device; every step
// of the job then samples.
static int sample_begin(GenJob& j, const SampleSetup& smp) {
  ttx_session* s = j.s;
  const int R = j.g.k.B;
  hipLaunchKernelGGL(k_sample_params, dim3(1), dim3(64), 0, j.st, s->smp_prm.as<SampleBlock>(), smp.blk);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sample_init, dim3(cdiv(R, 256)), dim3(256), 0, j.st, s->smp_key.as<unsigned long long>(),
                     s->smp_sample.as<unsigned>(), s->smp_done.as<int>(), s->smp_src_of.as<int>(), smp.d_row_keys, R, smp.n);
  HIP_TRY(hipGetLastError());
  StepCtx& k = j.g.k;
  k.src_of = s->smp_src_of.as<int>();
  k.want_sample = !smp.spec;
  k.want_sample_step = smp.spec;
  k.sample.key = s->smp_key.as<unsigned long long>(); k.sample.sample = s->smp_sample.as<unsigned>();
  k.sample.done = s->smp_done.as<int>(); k.sample.front = s->front.as<int>(); k.sample.prm = s->smp_prm.as<SampleBlock>();
  ConstraintTabs t;                                  // decoder row -> source: the map k_sample_init wrote
  TTX_TRY(constraints_upload(s, j.st, smp, k.max_len, k.p.pad_token, s->pfx_len.as<int>(), k.src_of, k.src_of, &t));
  k.bias = t.bias; k.syntax = t.syntax;
  if (smp.tabled()) {
    hipLaunchKernelGGL(k_prefix_rows, dim3(cdiv(R, 256)), dim3(256), 0, j.st, s->pfx_len_src.as<int>(), s->smp_src_of.as<int>(),
                       s->pfx_len.as<int>(), R);
    HIP_TRY(hipGetLastError());
    if (smp.proposed) { k.prop = t.pfx; k.prop_ctx = smp.prop_ctx; }      // offered: the sampling kernels see no table
    else k.sample.pfx = t.pfx;
    if (smp.spec) {                                  // draft 0 of every row as gen_start left it, before any step rewrites it
      HIP_TRY(hipMemcpy2DAsync(s->pfx_draft0.p, (size_t)k.D * 4, s->drafts.p, (size_t)k.N * k.D * 4, (size_t)k.D * 4, (size_t)R,
                               hipMemcpyDeviceToDevice, j.st));
      k.pfx_draft0 = s->pfx_draft0.as<int>();
    }
  }
  return TTX_OK;
}

// The batches of one generate call (validated by the caller) under drive_sessions: each session decodes the next batch of the list
// whenever it has finished one; a turn enqueues the next verify step of a session that has published its previous one (one step
// in flight per session, no stream synchronisation inside the loop).  `greedy` and `smp` are the single-session calls'.
static int generate_batches(ttx_session** sessions, int n_sessions, int n_batches, const int64_t* const* d_src, const int* B,
                            const int* Ls, const ttx_gen_params* p, int64_t* const* d_out, int16_t* const* d_traj,
                            int32_t* const* d_fin, ttx_gen_stats* stats, void* stream, bool greedy, const SampleSetup* smp) {
  std::vector<GenJob> jobs(n_sessions);
  const int D1 = greedy ? 1 : p->draft_len + 1;
  int next = 0, rc_batch = TTX_OK;               // next batch of the list; the first error a batch's own result carried
  const auto turn = [&](int i) -> int {
    GenJob& j = jobs[i];
    ttx_session* s = sessions[i];
    volatile HostInfo* hi = s->host_info;
    if (j.phase == 0) {
      if (next >= n_batches) return TURN_FINISHED;
      j.batch = next++;
      if (smp) TTX_TRY(sample_ensure(s, s->own_stream, (size_t)B[j.batch], *smp, p));
      TTX_TRY(gen_start(j, s, s->own_stream, d_src[j.batch], B[j.batch], Ls[j.batch], p, d_out[j.batch], stats ? &stats[j.batch] : nullptr,
                        greedy, d_traj ? d_traj[j.batch] : nullptr, d_traj ? d_fin[j.batch] : nullptr, smp ? smp->n : 1, smp && smp->spec));
      if (smp) TTX_TRY(sample_begin(j, *smp));
      return TURN_PROGRESSED;
    }
    if (j.phase == 1) {
      // loop init publishes no step: the stream has run it once it is idle; from then on the accept kernel publishes
      if (j.launched == 0 ? hipStreamQuery(s->own_stream) != hipSuccess : (!hi->stop && hi->steps_done < j.launched)) return TURN_WAITING;
      if (hi->stop) {                            // set by the accept kernel (or by loop init): nothing further to enqueue
        TTX_TRY(gen_finish_enqueue(j));
        return TURN_PROGRESSED;
      }
      if (j.launched > p->max_len + 2) return fail(TTX_ERR_HIP, "decode loop failed to terminate");
      TTX_TRY(gen_launch_step(j, hi->width + D1));
      return TURN_PROGRESSED;
    }
    if (hipEventQuery(s->ev_done) != hipSuccess) return TURN_IDLE;
    const int rc = gen_finish_collect(j);        // a batch the reference fails on does not end the other batches
    if (rc_batch == TTX_OK) rc_batch = rc;
    return TURN_PROGRESSED;
  };
  const int rc = drive_sessions(sessions, n_sessions, false, stream, [](int) { return TTX_OK; }, turn);
  return rc != TTX_OK ? rc : rc_batch;      // what ended the call (a hang, a failed launch) before what a batch reported
}

// A single-session generate call: one session, one batch.
static int generate_one(ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_gen_params* p, int64_t* d_out,
                        ttx_gen_stats* stats, void* stream, bool greedy, const SampleSetup* smp) {
  TTX_TRY(gen_validate(s, d_src, B, Ls, p, d_out, greedy));
  return generate_batches(&s, 1, 1, &d_src, &B, &Ls, p, &d_out, nullptr, nullptr, stats, stream, greedy, smp);
}

extern "C" int ttx_greedy_speculative_generate(ttx_session* s, const int64_t* d_src, int B, int Ls,
                                               const ttx_gen_params* p, int64_t* d_out, ttx_gen_stats* stats,
                                               void* stream) {
  return generate_one(s, d_src, B, Ls, p, d_out, stats, stream, false, nullptr);
}

extern "C" int ttx_greedy_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_gen_params* p,
                                   int64_t* d_out, ttx_gen_stats* stats, void* stream) {
  return generate_one(s, d_src, B, Ls, p, d_out, stats, stream, true, nullptr);
}

// The SampleBlock of a call, or TTX_ERR_INVALID: temperature >= 0 and finite (0: greedy), top_k 0 or 1..32, top_p in (0, 1].  A call
// that gives only top_p < 1 runs with top_k = 32.
static int sample_block(const char* who, const ttx_sample_params* p, SampleBlock* out) {
  if (!(p->temperature >= 0.0f) || !std::isfinite(p->temperature))
    return fail(TTX_ERR_INVALID, std::string(who) + ": temperature must be finite and >= 0");
  if (p->top_k < 0 || p->top_k > SAMPLE_MAX_KEEP) return fail(TTX_ERR_INVALID, std::string(who) + ": top_k must be 0 or in [1, 32]");
  if (!(p->top_p > 0.0f) || !(p->top_p <= 1.0f)) return fail(TTX_ERR_INVALID, std::string(who) + ": top_p must be in (0, 1]");
  SampleBlock b{};
  b.seed = p->seed;
  b.greedy = p->temperature == 0.0f ? 1 : 0;
  b.inv_T = b.greedy ? 0.0f : 1.0f / p->temperature;
  b.top_p = p->top_p;
  b.top_k = (p->top_k == 0 && p->top_p < 1.0f) ? SAMPLE_MAX_KEEP : p->top_k;
  b.pad = p->pad_token; b.eos = p->eos_token;
  if (!b.greedy && !(b.inv_T > 0.0f && std::isfinite(b.inv_T)))
    return fail(TTX_ERR_INVALID, std::string(who) + ": 1 / temperature is not a positive finite fp32");
  *out = b;
  return TTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Log-probability of hypotheses under the sampling distribution: csrc/ttx_logq.hip.h.
struct LogqOut {
  float* tok_logq; float* logq; int32_t* first_outside; int32_t* rank; int32_t* n_kept; int32_t* length; uint8_t* finished;
};

// The distribution of a call as the sampler would run it (sample_block: its limits, its inv_T, top_p < 1 alone runs with top_k 32).
static int logq_block(const char* who, const ttx_dist* d, SampleBlock* out) {
  if (!d) return fail(TTX_ERR_INVALID, std::string(who) + ": null distribution");
  ttx_sample_params p{};
  p.temperature = d->temperature; p.top_k = d->top_k; p.top_p = d->top_p;
  return sample_block(who, &p, out);
}

static bool logq_is_model(const SampleBlock& b, const int32_t* forced_len) {
  return !b.greedy && b.inv_T == 1.0f && b.top_k == 0 && !forced_len;
}

// ONE launch of k_hyp_logq, the VPL chosen as the sampler's kernels choose it.
static int launch_logq(ttx_session* s, hipStream_t st, const float* logits, const int64_t* hyp, int ld_hyp, int R, int W, int V, int pad,
                       int eos, const SampleBlock& b, const int32_t* forced_len, const LogqOut& o) {
  LogqArgs a{};
  a.logits = logits; a.hyp = hyp; a.forced_len = forced_len; a.tok_logq = o.tok_logq; a.logq = o.logq;
  a.first_outside = o.first_outside; a.rank = o.rank; a.n_kept = o.n_kept; a.length = o.length; a.finished = o.finished;
  a.ld_hyp = ld_hyp; a.W = W; a.V = V; a.pad = pad; a.eos = eos;
  a.inv_T = b.greedy ? 1.0f : b.inv_T; a.top_p = b.top_p; a.top_k = b.top_k; a.greedy = b.greedy;
  if (!a.tok_logq) {                      // the sum reads the per-token values back: session scratch when the caller wants none
    TTX_TRY(ensure(s->lq_tok, (size_t)R * (W - 1) * sizeof(float), st));
    a.tok_logq = s->lq_tok.as<float>();
  }
  const dim3 grid(R), block(LOGQ_THREADS);
  if (V <= 64) hipLaunchKernelGGL((k_hyp_logq<1>), grid, block, 0, st, a);
  else if (V <= 128) hipLaunchKernelGGL((k_hyp_logq<2>), grid, block, 0, st, a);
  else if (V <= 256) hipLaunchKernelGGL((k_hyp_logq<4>), grid, block, 0, st, a);
  else if (V <= 512) hipLaunchKernelGGL((k_hyp_logq<8>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((k_hyp_logq<16>), grid, block, 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// k_logit_bias on teacher-forced logits [R, T, V] of R hypothesis rows, N per source: logits row r * T + t belongs to source r / N.
static int bias_scored_logits(hipStream_t st, float* logits, int R, int T, int V, int N, const float* d_bias, int ld_bias) {
  LogitBiasArgs a{};
  a.logits = logits; a.V = V; a.M = R * T; a.tab = LogitBiasTab{d_bias, ld_bias, nullptr}; a.rows_per_src = N * T;
  return launch_logit_bias(st, a, false);
}

// k_syntax_mask on teacher-forced logits [R, T, V]: row r * T + t takes the prefix hyp[r][1 .. t] (k_hyp_logq's positions).
static int syntax_scored_logits(ttx_session* s, hipStream_t st, float* logits, int R, int T, int V, const int64_t* d_hyp, int ld_hyp,
                                const signed char* cls, int max_len, int eos) {
  SyntaxArgs a{};
  a.logits = logits; a.V = V; a.M = R * T; a.cls = cls; a.max_len = max_len; a.eos = eos; a.hyp = d_hyp; a.ld_hyp = ld_hyp; a.T = T;
  TTX_TRY(launch_syntax_mask(st, a, false));
  s->syntax_launches += 1;
  return TTX_OK;
}

// The syntax argument of a scoring call over rows of W columns: max_len 0 is W; otherwise at least 2.
static int syntax_validate_scored(const char* who, const ttx_syntax* syn, int W, const signed char** cls, int* max_len) {
  *cls = nullptr; *max_len = W;
  if (!syn || !syn->d_cls) return TTX_OK;
  if (syn->max_len != 0 && syn->max_len < 2) return fail(TTX_ERR_INVALID, std::string(who) + ": ttx_syntax.max_len must be 0 or at least 2");
  if (syn->max_len) *max_len = syn->max_len;
  *cls = reinterpret_cast<const signed char*>(syn->d_cls);
  return TTX_OK;
}

// The constraints of a scoring call: the bias [R / N][ld_bias] of N hypothesis rows per source and the syntax argument, null for none.
struct ScoreConstraints { const float* d_bias; int ld_bias; int N; const ttx_syntax* syntax; };

static int hypothesis_logq(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad, int eos,
                           const ttx_dist* dist, const int32_t* d_forced_len, const ScoreConstraints& c, const LogqOut& o, void* stream) {
  if (!s) return session_required("ttx_hypothesis_logq");
  const float* d_bias = c.d_bias;
  const int ld_bias = c.ld_bias, N = c.N;
  const signed char* cls; int syn_len;
  TTX_TRY(syntax_validate_scored("ttx_hypothesis_logq_syntax", c.syntax, W, &cls, &syn_len));
  if (!d_logits || !d_hyp || !o.logq || !o.length) return fail(TTX_ERR_INVALID, "bad argument to ttx_hypothesis_logq");
  TTX_TRY(check_score_shapes(s, R, W, V, "ttx_hypothesis_logq"));
  if (d_bias && (ld_bias < V || N < 1 || R % N != 0))
    return fail(TTX_ERR_INVALID, "ttx_hypothesis_logq_bias: ld_bias must be at least V and R a multiple of the rows per source");
  SampleBlock b{};
  TTX_TRY(logq_block("ttx_hypothesis_logq", dist, &b));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  if (d_bias || cls) {                    // the caller's logits stay as they are: the biased / masked copy lives in session scratch
    const size_t bytes = (size_t)R * (W - 1) * V * sizeof(float);
    TTX_TRY(ensure(s->ev_logits, bytes, st));
    HIP_TRY(hipMemcpyAsync(s->ev_logits.p, d_logits, bytes, hipMemcpyDeviceToDevice, st));
    if (d_bias) {
      TTX_TRY(bias_scored_logits(st, s->ev_logits.as<float>(), R, W - 1, V, N, d_bias, ld_bias));
      s->logit_bias_launches += 1;
    }
    if (cls) TTX_TRY(syntax_scored_logits(s, st, s->ev_logits.as<float>(), R, W - 1, V, d_hyp, W, cls, syn_len, eos));
    d_logits = s->ev_logits.as<float>();
  }
  return launch_logq(s, st, d_logits, d_hyp, W, R, W, V, pad, eos, b, d_forced_len, o);
}

extern "C" int ttx_hypothesis_logq(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad, int eos,
                                   const ttx_dist* dist, const int32_t* d_forced_len, float* d_tok_logq, float* d_logq,
                                   int32_t* d_first_outside, int32_t* d_rank, int32_t* d_n_kept, int32_t* d_length,
                                   uint8_t* d_finished, void* stream) {
  return hypothesis_logq(s, d_logits, d_hyp, R, W, V, pad, eos, dist, d_forced_len, ScoreConstraints{nullptr, 0, 1, nullptr},
                         LogqOut{d_tok_logq, d_logq, d_first_outside, d_rank, d_n_kept, d_length, d_finished}, stream);
}

extern "C" int ttx_hypothesis_logq_bias(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad, int eos,
                                        const ttx_dist* dist, const int32_t* d_forced_len, const float* d_bias, int ld_bias, int N,
                                        float* d_tok_logq, float* d_logq, int32_t* d_first_outside, int32_t* d_rank, int32_t* d_n_kept,
                                        int32_t* d_length, uint8_t* d_finished, void* stream) {
  return hypothesis_logq(s, d_logits, d_hyp, R, W, V, pad, eos, dist, d_forced_len, ScoreConstraints{d_bias, ld_bias, N, nullptr},
                         LogqOut{d_tok_logq, d_logq, d_first_outside, d_rank, d_n_kept, d_length, d_finished}, stream);
}

// ttx_hypothesis_logq_bias under a syntax constraint: k_syntax_mask on the (biased) copy of the logits before the log q stage.
extern "C" int ttx_hypothesis_logq_syntax(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad, int eos,
                                          const ttx_dist* dist, const int32_t* d_forced_len, const float* d_bias, int ld_bias, int N,
                                          const ttx_syntax* syntax, float* d_tok_logq, float* d_logq, int32_t* d_first_outside,
                                          int32_t* d_rank, int32_t* d_n_kept, int32_t* d_length, uint8_t* d_finished, void* stream) {
  return hypothesis_logq(s, d_logits, d_hyp, R, W, V, pad, eos, dist, d_forced_len, ScoreConstraints{d_bias, ld_bias, N, syntax},
                         LogqOut{d_tok_logq, d_logq, d_first_outside, d_rank, d_n_kept, d_length, d_finished}, stream);
}

static int score_proposal(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W,
                          int eos, const ttx_dist* dist, const int32_t* d_forced_len, float* d_logits, float* d_tok_logp,
                          float* d_score, float* d_tok_logq, float* d_logq, int32_t* d_first_outside, int32_t* d_rank,
                          int32_t* d_n_kept, int32_t* d_length, uint8_t* d_finished, void* stream, const ScoreConstraints& sc) {
  if (!s) return session_required("ttx_score_proposal");
  const float* d_bias = sc.d_bias;
  const int ld_bias = sc.ld_bias;
  const signed char* cls; int syn_len;
  TTX_TRY(syntax_validate_scored("ttx_score_proposal_syntax", sc.syntax, W, &cls, &syn_len));
  if (d_bias && ld_bias < s->m->cfg.vocab_size) return fail(TTX_ERR_INVALID, "ttx_score_proposal_bias: ld_bias must be at least the vocabulary");
  if (!d_src || !d_hyp || !d_logq || !d_length || B <= 0 || N <= 0 || Ls <= 0)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_score_proposal");
  if (d_tok_logp && !d_score) return fail(TTX_ERR_INVALID, "ttx_score_proposal: d_tok_logp needs d_score");
  if (ld_hyp < W) return fail(TTX_ERR_INVALID, "ttx_score_proposal: row stride ld_hyp smaller than W");
  const ttx_config& c = s->m->cfg;
  TTX_TRY(check_score_shapes(s, (long long)B * N, W, c.vocab_size, "ttx_score_proposal"));
  if (Ls > c.max_positions) return fail(TTX_ERR_INVALID, "source longer than the positional table");
  SampleBlock b{};
  TTX_TRY(logq_block("ttx_score_proposal", dist, &b));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->m->device));
  const int R = B * N, T = W - 1, V = c.vocab_size, pad = c.pad_token;
  if (!d_logits) {
    TTX_TRY(ensure(s->ev_logits, (size_t)R * T * V * sizeof(float), st));
    d_logits = s->ev_logits.as<float>();
  }
  TTX_TRY(score_forward(s, st, d_src, B, Ls, d_hyp, ld_hyp, N, W, d_logits));
  if (d_bias || cls) {
    // p before q, from one pass: k_hyp_score reads the raw logits, k_logit_bias and k_syntax_mask then rewrite them in place (a
    // caller's d_logits receives the biased, masked values), and k_hyp_logq reads what the constrained sampler's consumer reads
    if (d_score) TTX_TRY(launch_score(s, st, d_logits, d_hyp, ld_hyp, R, W, V, pad, eos, d_tok_logp, d_score, d_length, d_finished));
    if (d_bias) {
      TTX_TRY(bias_scored_logits(st, d_logits, R, T, V, N, d_bias, ld_bias));
      s->logit_bias_launches += 1;
    }
    if (cls) TTX_TRY(syntax_scored_logits(s, st, d_logits, R, T, V, d_hyp, ld_hyp, cls, syn_len, eos));
    return launch_logq(s, st, d_logits, d_hyp, ld_hyp, R, W, V, pad, eos, b, d_forced_len,
                       LogqOut{d_tok_logq, d_logq, d_first_outside, d_rank, d_n_kept, d_length, d_finished});
  }
  if (logq_is_model(b, d_forced_len)) {
    // q is the model's own distribution: ONE launch of k_hyp_score gives the values, so that they are ttx_score_hypotheses' bit
    // for bit; with d_score set they are copied, not computed twice.  first_outside follows from them (k_logq_first_outside);
    // k_hyp_logq runs for rank / n_kept alone.
    const float* tok = nullptr;
    if (d_score) {
      TTX_TRY(launch_score(s, st, d_logits, d_hyp, ld_hyp, R, W, V, pad, eos, d_tok_logp, d_score, d_length, d_finished));
      tok = d_tok_logp ? d_tok_logp : s->ev_nll.as<float>();
      if (d_tok_logq) HIP_TRY(hipMemcpyAsync(d_tok_logq, tok, (size_t)R * T * sizeof(float), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_logq, d_score, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else {
      TTX_TRY(launch_score(s, st, d_logits, d_hyp, ld_hyp, R, W, V, pad, eos, d_tok_logq, d_logq, d_length, d_finished));
      tok = d_tok_logq ? d_tok_logq : s->ev_nll.as<float>();
    }
    if (d_first_outside) {
      hipLaunchKernelGGL(k_logq_first_outside, dim3(cdiv(R, 4)), dim3(256), 0, st, tok, d_length, d_first_outside, R, T);
      HIP_TRY(hipGetLastError());
    }
    if (!d_rank && !d_n_kept) return TTX_OK;
    return launch_logq(s, st, d_logits, d_hyp, ld_hyp, R, W, V, pad, eos, b, nullptr,
                       LogqOut{nullptr, nullptr, nullptr, d_rank, d_n_kept, nullptr, nullptr});
  }
  if (d_score) TTX_TRY(launch_score(s, st, d_logits, d_hyp, ld_hyp, R, W, V, pad, eos, d_tok_logp, d_score, d_length, d_finished));
  return launch_logq(s, st, d_logits, d_hyp, ld_hyp, R, W, V, pad, eos, b, d_forced_len,
                     LogqOut{d_tok_logq, d_logq, d_first_outside, d_rank, d_n_kept, d_length, d_finished});
}

extern "C" int ttx_score_proposal(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W,
                                  int eos, const ttx_dist* dist, const int32_t* d_forced_len, float* d_logits, float* d_tok_logp,
                                  float* d_score, float* d_tok_logq, float* d_logq, int32_t* d_first_outside, int32_t* d_rank,
                                  int32_t* d_n_kept, int32_t* d_length, uint8_t* d_finished, void* stream) {
  return score_proposal(s, d_src, B, Ls, d_hyp, ld_hyp, N, W, eos, dist, d_forced_len, d_logits, d_tok_logp, d_score, d_tok_logq, d_logq,
                        d_first_outside, d_rank, d_n_kept, d_length, d_finished, stream, ScoreConstraints{nullptr, 0, N, nullptr});
}

extern "C" int ttx_score_proposal_bias(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W,
                                       int eos, const ttx_dist* dist, const int32_t* d_forced_len, const float* d_bias, int ld_bias,
                                       float* d_logits, float* d_tok_logp, float* d_score, float* d_tok_logq, float* d_logq,
                                       int32_t* d_first_outside, int32_t* d_rank, int32_t* d_n_kept, int32_t* d_length,
                                       uint8_t* d_finished, void* stream) {
  return score_proposal(s, d_src, B, Ls, d_hyp, ld_hyp, N, W, eos, dist, d_forced_len, d_logits, d_tok_logp, d_score, d_tok_logq, d_logq,
                        d_first_outside, d_rank, d_n_kept, d_length, d_finished, stream, ScoreConstraints{d_bias, ld_bias, N, nullptr});
}

// ttx_score_proposal_bias under a syntax constraint (a null `syntax` is that call).
extern "C" int ttx_score_proposal_syntax(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W,
                                         int eos, const ttx_dist* dist, const int32_t* d_forced_len, const float* d_bias, int ld_bias,
                                         const ttx_syntax* syntax, float* d_logits, float* d_tok_logp, float* d_score, float* d_tok_logq,
                                         float* d_logq, int32_t* d_first_outside, int32_t* d_rank, int32_t* d_n_kept, int32_t* d_length,
                                         uint8_t* d_finished, void* stream) {
  return score_proposal(s, d_src, B, Ls, d_hyp, ld_hyp, N, W, eos, dist, d_forced_len, d_logits, d_tok_logp, d_score, d_tok_logq, d_logq,
                        d_first_outside, d_rank, d_n_kept, d_length, d_finished, stream, ScoreConstraints{d_bias, ld_bias, N, syntax});
}

// The options of a form that spells them out as arguments; a form that takes none passes NO_OPTS, as a null `o` does.
static const ttx_sample_opts NO_OPTS{};
static ttx_sample_opts opts_of(const int64_t* d_prefix, int ld_prefix, const int32_t* h_prefix_len, const int64_t* d_proposal,
                               int ld_proposal, const int32_t* h_proposal_len) {
  ttx_sample_opts o{};
  o.d_prefix = d_prefix; o.ld_prefix = ld_prefix; o.h_prefix_len = h_prefix_len;
  o.d_proposal = d_proposal; o.ld_proposal = ld_proposal; o.h_proposal_len = h_proposal_len;
  return o;
}

// The body of every form of ttx_sample_generate; `form` names the one that was called where a refusal says so.
static int sample_generate(const char* form, ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                           const ttx_sample_params* p, const ttx_sample_opts& o, const ttx_syntax* syn, int64_t* d_out,
                           ttx_gen_stats* stats, void* stream) {
  if (o.h_proposal_len) return fail(TTX_ERR_INVALID, std::string(form) + ": the plain sampler verifies no drafts and takes no proposal");
  if (!s || !p) return fail(TTX_ERR_INVALID, "bad argument to a generate call");
  if (s->m->cfg.vocab_size > SAMPLE_MAX_V) return fail(TTX_ERR_INVALID, "ttx_sample_generate: vocabularies above 1024 are not supported");
  if (p->num_samples < 1) return fail(TTX_ERR_INVALID, "ttx_sample_generate: num_samples must be at least 1");
  SampleSetup smp{};
  TTX_TRY(sample_block("ttx_sample_generate", p, &smp.blk));
  if (B > 0 && (long long)B * p->num_samples * ((long long)std::max(p->max_len, 0) + 2) >= (1ll << 31))
    return fail(TTX_ERR_INVALID, "ttx_sample_generate: B * num_samples * (max_len + 2) must stay below 2^31");
  smp.n = p->num_samples; smp.d_row_keys = d_row_keys;
  TTX_TRY(constraints_validate(Who("ttx_sample_generate", "ttx_sample_generate", "ttx_sample_generate", "ttx_sample_generate_syntax"), s, o,
                               syn, std::max(B, 0), p->max_len, &smp));
  ttx_gen_params g{};
  g.max_len = p->max_len; g.draft_len = 0; g.n_drafts = 1; g.pad_token = p->pad_token; g.bos_token = p->bos_token;
  g.eos_token = p->eos_token; g.replace_token = p->pad_token; g.want_logits = 0;
  if (B <= 0) return fail(TTX_ERR_INVALID, "bad argument to a generate call");
  const int rc = generate_one(s, d_src, B * p->num_samples, Ls, &g, d_out, stats, stream, true, &smp);
  if (rc == TTX_OK && stats) stats->src_tokens_padded = (long long)B * Ls;    // the encoder ran once per source
  return rc;
}

extern "C" int ttx_sample_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                   const ttx_sample_params* p, int64_t* d_out, ttx_gen_stats* stats, void* stream) {
  return sample_generate("ttx_sample_generate", s, d_src, B, Ls, d_row_keys, p, NO_OPTS, nullptr, d_out, stats, stream);
}

extern "C" int ttx_sample_generate_prefix(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                          const ttx_sample_params* p, const int64_t* d_prefix, int ld_prefix, const int32_t* h_prefix_len,
                                          int64_t* d_out, ttx_gen_stats* stats, void* stream) {
  return sample_generate("ttx_sample_generate_prefix", s, d_src, B, Ls, d_row_keys, p, opts_of(d_prefix, ld_prefix, h_prefix_len, nullptr, 0, nullptr),
                         nullptr, d_out, stats, stream);
}

// The form that takes every option of the plain sampler: the prefix of ttx_sample_generate_prefix and the per-source logit bias.
extern "C" int ttx_sample_generate_ex(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                      const ttx_sample_params* p, const ttx_sample_opts* o, int64_t* d_out, ttx_gen_stats* stats,
                                      void* stream) {
  return sample_generate("ttx_sample_generate_ex", s, d_src, B, Ls, d_row_keys, p, o ? *o : NO_OPTS, nullptr, d_out, stats, stream);
}

// The general form: ttx_sample_generate_ex under a syntax constraint (a null `syntax`, or a null table, is that call, launch for launch).
extern "C" int ttx_sample_generate_syntax(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                          const ttx_sample_params* p, const ttx_sample_opts* o, const ttx_syntax* syntax, int64_t* d_out,
                                          ttx_gen_stats* stats, void* stream) {
  return sample_generate("ttx_sample_generate_syntax", s, d_src, B, Ls, d_row_keys, p, o ? *o : NO_OPTS, syntax, d_out, stats, stream);
}

// What the speculative sampling calls refuse with TTX_ERR_INVALID whatever code gen_validate would give (nothing of these calls is
// the reference's), over `rows` decoder rows in one loop; then the call's SampleSetup and the loop's parameters.
static int sample_spec_validate(const char* who, const ttx_session* s, const ttx_sample_spec_params* p, long long rows, SampleSetup* smp,
                                ttx_gen_params* g) {
  const ttx_sample_params& sp = p->sample;
  if (s->m->cfg.vocab_size > SAMPLE_MAX_V) return fail(TTX_ERR_INVALID, std::string(who) + ": vocabularies above 1024 are not supported");
  if (sp.num_samples < 1) return fail(TTX_ERR_INVALID, std::string(who) + ": num_samples must be at least 1");
  TTX_TRY(sample_block(who, &sp, &smp->blk));
  if (p->n_drafts < 1) return fail(TTX_ERR_INVALID, std::string(who) + ": n_drafts must be at least 1");
  if (sp.max_len < 1) return fail(TTX_ERR_INVALID, std::string(who) + ": max_len must be positive");
  if (p->draft_len < 1 || p->draft_len > sp.max_len) return fail(TTX_ERR_INVALID, std::string(who) + ": draft_len must lie in [1, max_len]");
  if (sp.pad_token == p->replace_token || sp.eos_token == p->replace_token || sp.eos_token == sp.pad_token)
    return fail(TTX_ERR_INVALID, std::string(who) + ": pad, eos and replace tokens must be pairwise different");
  if (rows * ((long long)sp.max_len + p->draft_len + 2) >= (1ll << 31) ||
      rows * step_rps(p->n_drafts, p->draft_len) * (long long)s->m->cfg.vocab_size >= (1ll << 31))
    return fail(TTX_ERR_INVALID, std::string(who) + ": B * num_samples * (max_len + draft_len + 2) and the step's logits must stay below 2^31 elements");
  smp->n = sp.num_samples; smp->spec = true;
  g->max_len = sp.max_len; g->draft_len = p->draft_len; g->n_drafts = p->n_drafts; g->pad_token = sp.pad_token; g->bos_token = sp.bos_token;
  g->eos_token = sp.eos_token; g->replace_token = p->replace_token; g->want_logits = 0;
  return TTX_OK;
}

// Speculative seeded sampling: the greedy-speculative loop over R = B * n decoder rows with the keyed draw where the argmax stands
// (k_sample_step, k_sample_accept).  A draft token is accepted iff it is the token the plain sampler emits at its position, so the
// committed rows are ttx_sample_generate's.
static int sample_speculative_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                       const ttx_sample_spec_params* p, const ttx_sample_opts& o, const ttx_syntax* syn, int64_t* d_out,
                                       ttx_gen_stats* stats, void* stream) {
  const char* who = "ttx_sample_speculative_generate";
  if (!s || !p) return fail(TTX_ERR_INVALID, "bad argument to a generate call");
  SampleSetup smp{};
  ttx_gen_params g{};
  const long long R = (long long)std::max(B, 0) * std::max(p->sample.num_samples, 0);
  TTX_TRY(sample_spec_validate(who, s, p, R, &smp, &g));
  if (B <= 0) return fail(TTX_ERR_INVALID, "bad argument to a generate call");
  smp.d_row_keys = d_row_keys;
  TTX_TRY(constraints_validate(who, s, o, syn, B, g.max_len, &smp));
  const int rc = generate_one(s, d_src, (int)R, Ls, &g, d_out, stats, stream, false, &smp);
  if (rc == TTX_OK && stats) stats->src_tokens_padded = (long long)B * Ls;    // the encoder ran once per source
  return rc;
}

extern "C" int ttx_sample_speculative_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                               const ttx_sample_spec_params* p, int64_t* d_out, ttx_gen_stats* stats, void* stream) {
  return sample_speculative_generate(s, d_src, B, Ls, d_row_keys, p, NO_OPTS, nullptr, d_out, stats, stream);
}

// The prompted form: the prefix rides in as draft 0 (k_prefix_drafts), ceil(len / (draft_len + 1)) steps for len forced tokens.
extern "C" int ttx_sample_speculative_generate_prefix(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                                      const ttx_sample_spec_params* p, const int64_t* d_prefix, int ld_prefix,
                                                      const int32_t* h_prefix_len, int64_t* d_out, ttx_gen_stats* stats, void* stream) {
  return sample_speculative_generate(s, d_src, B, Ls, d_row_keys, p, opts_of(d_prefix, ld_prefix, h_prefix_len, nullptr, 0, nullptr), nullptr,
                                     d_out, stats, stream);
}

// The proposed form: the proposal is offered as draft 0 wherever it can be aligned with the row (k_proposal_drafts); no token changes.
extern "C" int ttx_sample_speculative_generate_proposal(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                                        const ttx_sample_spec_params* p, const int64_t* d_prefix, int ld_prefix,
                                                        const int32_t* h_prefix_len, const int64_t* d_proposal, int ld_proposal,
                                                        const int32_t* h_proposal_len, int64_t* d_out, ttx_gen_stats* stats,
                                                        void* stream) {
  return sample_speculative_generate(s, d_src, B, Ls, d_row_keys, p,
                                     opts_of(d_prefix, ld_prefix, h_prefix_len, d_proposal, ld_proposal, h_proposal_len), nullptr, d_out, stats,
                                     stream);
}

// The form that takes every option: prefix, proposal and the per-source logit bias (a null `o` is the plain call).
extern "C" int ttx_sample_speculative_generate_ex(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                                  const ttx_sample_spec_params* p, const ttx_sample_opts* o, int64_t* d_out,
                                                  ttx_gen_stats* stats, void* stream) {
  return sample_speculative_generate(s, d_src, B, Ls, d_row_keys, p, o ? *o : NO_OPTS, nullptr, d_out, stats, stream);
}

// The general form: ttx_sample_speculative_generate_ex under a syntax constraint.  The keyed draw of a draft position comes from the
// row masked for the prefix that includes the earlier draft tokens, so the committed rows are ttx_sample_generate_syntax's.
extern "C" int ttx_sample_speculative_generate_syntax(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                                      const ttx_sample_spec_params* p, const ttx_sample_opts* o, const ttx_syntax* syntax,
                                                      int64_t* d_out, ttx_gen_stats* stats, void* stream) {
  return sample_speculative_generate(s, d_src, B, Ls, d_row_keys, p, o ? *o : NO_OPTS, syntax, d_out, stats, stream);
}

// ------------------------------------------------------------------------------------------------
// Slot pool: continuous batching under the per-row rule.  A session owns `C` slots; whenever enough of them are free
// the next rows of the (length-sorted) work list are encoded and admitted, so the verify step keeps close to
// C * (1 + N*D) rows from the first step to the last instead of decaying with every retiring sequence, and there is
// no tail of half-empty groups.  The step graph has one shape per session (C, Ls_cap): captured once.
struct PoolJob {
  ttx_session* s = nullptr;
  hipStream_t st = nullptr;
  GenCtx g{};
  int C = 0, Ls_cap = 0;
  PoolState pool;           // launched: steps whose accept and commit are enqueued (pool_step, ttx_admit.h)
  PoolIo io{};
  long long src_tokens_padded = 0;
  long long admit_rows = 0; // TTX_ADMIT_ROWS: padded encoder rows at which a sub-chunk of an admission closes; 0: one chunk per admission
  // two-phase verify step (DESIGN.md "Two-phase verify step"): a free choice per step, both forms give the same bits
  bool two_phase = true;    // TTX_TWO_PHASE=0: every step in one pass
  long long min_rows = 800; // TTX_TWO_PHASE_MIN_ROWS: steps with fewer live rows (slots * RPS) run in one pass; 0: always split
  GenCtx g2{};              // accept and commit behind a split step: executed-row count, indirection of the K/V commit
  ProbeInfo* dev_probe = nullptr;   // device address of the session's pinned probe words
  int probes = 0;           // probes launched
  bool probe_pending = false;   // a probe is in flight; the step's second graph follows once it has published
  long long slot_steps = 0, matched_slot_steps = 0, split_steps = 0, skipped_draft_passes = 0;   // TTX_TWO_PHASE_STATS=1
  // draft select: the draft pass runs row 0 and the drafts whose first token matched, stored compacted
  bool draft_select = false;
  long long drafts_matched = 0;     // drafts run by the draft passes (draft select: the matching ones; else N per matching slot)
  long long rows_executed = 0;      // rows every step of this pool sent through the decoder, probes included
  long long unsplit_rows = 0;       // ... of which in steps that ran in one pass
  // sampling pool (ttx_sample_speculative_generate_pool; 0 / null: the greedy pool): decoder rows per source, the sources' keys
  int per_src = 0;
  const int64_t* d_row_keys = nullptr;
};

static int pool_sample_begin(PoolJob& j, const SampleSetup& smp);

// `smp` (null: the greedy pool): the sampling pool, whose slots carry a key and a sample id, whose steps draw with k_sample_step and
// accept with k_sample_accept, and which keeps no per-row trace (d_traj and d_fin are null).
static int pool_start(PoolJob& j, ttx_session* s, hipStream_t st, int C, int Ls_cap, const ttx_gen_params* p, int64_t* d_out,
                      int16_t* d_traj, int32_t* d_fin, const SampleSetup* smp) {
  const ttx_config& c = s->m->cfg;
  const int d = c.embedding_dim, Ld = c.num_decoder_layers;
  const int N = p->n_drafts, D = p->draft_len, D1 = D + 1, max_len = p->max_len;
  j.s = s; j.st = st; j.C = C; j.Ls_cap = Ls_cap; j.pool = PoolState{}; j.src_tokens_padded = 0;
  s->snap_step = 0;
  GenCtx& g = j.g;
  g = GenCtx{};
  g.k.B = C; g.k.Ls = Ls_cap; g.k.N = N; g.k.D = D; g.k.max_len = max_len; g.k.p = *p;
  g.k.Lc = max_len + D1;
  g.k.gen_ld = max_len + D + 2;
  const size_t Mmax = (size_t)C * step_rps(N, D);
  Needs need{st};
  need_source_slots(s, need, C, Ls_cap);
  need(s->drafts, (size_t)C * N * D * 4); need(s->drafts_new, (size_t)C * N * D * 4);
  need(s->gen, (size_t)C * g.k.gen_ld * 4);
  for (Buf* b : {&s->front, &s->act_idx, &s->haspad, &s->rstep, &s->row_of, &s->src_len, &s->new_slot}) need(*b, (size_t)C * 4);
  need(s->rec, (size_t)C * sizeof(CopyRec)); need(s->pool_io, sizeof(PoolIo));
  need(s->kcache, (size_t)Ld * C * g.k.Lc * d * 4); need(s->vcache, (size_t)Ld * C * g.k.Lc * d * 4);
  need_step_workspaces(s, need, Mmax, (size_t)C * Ls_cap);
  // read at the start of every pool call
  j.two_phase = true; j.min_rows = 800; j.probes = 0; j.probe_pending = false;
  j.slot_steps = j.matched_slot_steps = j.split_steps = j.skipped_draft_passes = 0;
  j.drafts_matched = j.rows_executed = j.unsplit_rows = 0;
  j.admit_rows = ADMIT_ROWS;
  if (const char* e = getenv("TTX_ADMIT_ROWS")) j.admit_rows = std::max(0, atoi(e));
  if (const char* e = getenv("TTX_TWO_PHASE")) j.two_phase = atoi(e) != 0;
  if (const char* e = getenv("TTX_TWO_PHASE_MIN_ROWS")) j.min_rows = std::max(0, atoi(e));
  // draft select needs the compacted-row mapping, which k_attn3 / k_attn3s have: head dimension 32, H % 4 == 0.  Models whose step
  // attention runs on k_attn2 / k_attn keep the all-drafts pass.
  j.draft_select = j.two_phase && d == c.num_heads * ATT_DH && c.num_heads % 4 == 0 && !s->attn_fallback && N <= 32 && D >= 1;
  if (const char* e = getenv("TTX_DRAFT_SELECT")) j.draft_select = j.draft_select && atoi(e) != 0;
  if (j.draft_select) {
    for (Buf* b : {&s->draft_mask, &s->row_base}) need(*b, (size_t)C * 4);
    need(s->row_map, Mmax * 4);
  }
  if (j.two_phase) {                                              // nothing may allocate inside a capture
    need(s->qkv_probe, (size_t)Ld * C * 3 * d * 4);
    for (Buf* b : {&s->pred_probe, &s->act2, &s->pos2}) need(*b, (size_t)C * 4);
    need(s->pred_draft, Mmax * 4); need(s->state2, 3 * sizeof(DecState));
  }
  if (smp) { need(s->smp_key, (size_t)C * 8); need(s->smp_sample, (size_t)C * 4); need(s->smp_prm, sizeof(SampleBlock)); }
  if (smp && smp->tabled()) need(s->pfx_src, (size_t)C * 4);          // the slots' own row-to-source maps, written at admission
  if (smp && smp->d_bias) need(s->lb_src, (size_t)C * 4);
  if (smp && need.rc == TTX_OK) need.rc = constraints_ensure(s, st, *smp, max_len, (size_t)C, (size_t)C * D, 0);
  TTX_TRY(need.rc);
  AcceptBlk* blk = nullptr;
  // the greedy pool keeps the session's reading of TTX_ACCEPT_SPREAD; the sampling pool reads it here, with its other switches
  // (unset: on), and that reading alone decides
  bool spread = s->accept_spread;
  if (smp) { const char* e = getenv("TTX_ACCEPT_SPREAD"); spread = e ? atoi(e) != 0 : true; }
  TTX_TRY(accept_blk_when(s, st, C, spread, &blk));
  s->graphs_current();

  s->ev_used = 0;
  HIP_TRY(hipEventRecord(s->ev_a, st));
  if (j.two_phase) {
    HIP_TRY(hipMemsetAsync(s->state2.p, 0, 3 * sizeof(DecState), st));
    s->probe_info->matches = 0; s->probe_info->probes_done = 0; s->probe_info->rows = 0;
    HIP_TRY(hipHostGetDevicePointer((void**)&j.dev_probe, (void*)s->probe_info, 0));
  }
  j.io = PoolIo{d_out, d_traj, d_fin, max_len + 1, 0};        // lives in the job until every stream has drained
  HIP_TRY(hipMemcpyAsync(s->pool_io.p, &j.io, sizeof(j.io), hipMemcpyHostToDevice, st));
  TTX_TRY(fill_loop_args(s, g, blk));
  g.la.row_rule = 1;
  g.la.pool = 1; g.la.rstep = s->rstep.as<int>(); g.la.row_of = s->row_of.as<int>(); g.la.io = s->pool_io.as<PoolIo>();
  g.k.src_len = s->src_len.as<int>();
  j.per_src = 0; j.d_row_keys = nullptr;
  if (smp) TTX_TRY(pool_sample_begin(j, *smp));
  j.g2 = g;
  if (j.two_phase) {
    j.g2.la.exec_rows = reinterpret_cast<const int*>(s->state2.as<DecState>() + 2);
    j.g2.kc.pos2 = s->pos2.as<int>(); j.g2.kc.qkv_probe = s->qkv_probe.as<float>(); j.g2.kc.probe_layer_stride = (long long)C * 3 * d;
    if (j.draft_select) { j.g2.kc.row_base = s->row_base.as<int>(); j.g2.kc.draft_mask = s->draft_mask.as<int>(); }
  }
  s->host_info->stop = 0; s->host_info->steps_done = 0; s->host_info->width = 1; s->host_info->n_active = 0;
  hipLaunchKernelGGL(k_pool_init, dim3(4), dim3(256), 0, st, g.la);
  HIP_TRY(hipGetLastError());
  j.pool.phase = 1;
  return TTX_OK;
}

// Encode R new rows (rows first_row .. first_row+R-1 of the caller's sorted matrix, Ls_new columns of it) and hand
// them free slots.
// Sampling pool: the R rows of d_src_rows are sources (first_row the first one's index); each is encoded once and fills
// j.per_src slots, rows first_row * per_src .. of d_out.
static int pool_admit(PoolJob& j, const int64_t* d_src_rows, int ld_src, int R, int Ls_new, int first_row, int64_t* d_out,
                      int16_t* d_traj, int32_t* d_fin) {
  ttx_session* s = j.s;
  hipStream_t st = j.st;
  const StepCtx& k = j.g.k;
  const int kv_row = s->m->cfg.num_decoder_layers * 2 * s->m->cfg.embedding_dim;
  const int per = std::max(1, j.per_src), rows = R * per, row0 = first_row * per;      // decoder rows of this admission
  TTX_TRY(encode_sources(s, st, d_src_rows, ld_src, R, Ls_new, s->valid_new.as<uint8_t>(), s->memkv_new.as<float>()));
  TTX_TRY(launch_make_drafts<int>(st, s->tok_src.as<int>(), Ls_new, 1, R, Ls_new - 1, k.N, k.D, k.p.eos_token, k.p.pad_token,
                                  k.p.replace_token, s->drafts_new.as<int>()));
  PoolAdmitArgs a{};
  a.st = s->state.as<DecState>(); a.act_idx = s->act_idx.as<int>(); a.front = s->front.as<int>(); a.haspad = s->haspad.as<int>();
  a.rstep = s->rstep.as<int>(); a.row_of = s->row_of.as<int>(); a.src_len = s->src_len.as<int>(); a.new_slot = s->new_slot.as<int>();
  a.host = j.g.la.host; a.B = j.C; a.N = k.N; a.D = k.D; a.R = rows; a.first_row = row0; a.Ls_new = Ls_new;
  if (j.per_src) {
    a.key = s->smp_key.as<unsigned long long>(); a.sample = s->smp_sample.as<unsigned>(); a.row_keys = j.d_row_keys;
    a.per_src = j.per_src; a.first_src = first_row;
    if (step_tab(k).tok) { a.pfx_src = s->pfx_src.as<int>(); a.pfx_len = s->pfx_len.as<int>(); a.pfx_len_of_src = s->pfx_len_src.as<int>(); }
    if (k.bias.val) a.bias_src = s->lb_src.as<int>();
  }
  hipLaunchKernelGGL(k_pool_admit, dim3(1), dim3(256), (size_t)j.C * 4, st, a);
  HIP_TRY(hipGetLastError());
  PoolFillArgs f{};
  f.new_slot = s->new_slot.as<int>(); f.R = rows; f.gen = s->gen.as<int>(); f.gen_ld = k.gen_ld; f.bos = k.p.bos_token; f.pad = k.p.pad_token;
  f.drafts = s->drafts.as<int>(); f.drafts_new = s->drafts_new.as<int>(); f.nd = k.N * k.D;
  f.src_valid = s->src_valid.as<uint8_t>(); f.valid_new = s->valid_new.as<uint8_t>(); f.Ls_cap = j.Ls_cap; f.Ls_new = Ls_new;
  f.memkv = s->memkv.as<float>(); f.memkv_new = s->memkv_new.as<float>(); f.kv_row = kv_row;
  f.out_rows = d_out; f.traj_rows = d_traj; f.fin_rows = d_fin; f.max_len = k.max_len; f.traj_ld = k.max_len + 1; f.first_row = row0;
  f.per_src = j.per_src;
  if (step_tab(k).tok) { f.draft0 = s->pfx_draft0.as<int>(); f.D = k.D; }
  hipLaunchKernelGGL(k_pool_fill, dim3(rows, 1 + Ls_new), dim3(256), 0, st, f);
  HIP_TRY(hipGetLastError());
  j.src_tokens_padded += (long long)R * Ls_new;
  return TTX_OK;
}

// Key of one graph's worth of a pool step (`phase`: GraphKey in ttx_internal.h); the pool's steps see every key of a slot.
// The sampling pool has a site of its own, and its keys end with the form of the accept step (1: the pair), which it reads from
// the environment per call.
static GraphKey pool_key(const PoolJob& j, const StepCtx& k, int variant, int phase) {
  // a biased or a constrained step is never replayed for a call without the bias or the constraint
  const int biased = (k.bias.val ? GS_LOGIT_BIAS : 0) | (k.syntax ? GS_SYNTAX : 0);
  if (k.want_sample_step && k.prop.tok)              // a proposed pool: a site of its own, the key ends with the context length
    return GraphKey{GS_STEP_POOL_SAMPLE_PROPOSAL | biased, k.B, k.Ls, k.N, k.D, k.max_len, k.max_len, variant, phase, j.g.la.blk ? 1 : 0, k.prop_ctx};
  if (k.want_sample_step)
    return GraphKey{(k.sample.pfx.tok ? GS_STEP_POOL_SAMPLE_PREFIX : GS_STEP_POOL_SAMPLE) | biased, k.B, k.Ls, k.N, k.D, k.max_len, k.max_len, variant, phase, j.g.la.blk ? 1 : 0};
  return GraphKey{GS_STEP_POOL, k.B, k.Ls, k.N, k.D, k.max_len, k.max_len, variant, phase};
}

// One verify step of the pool.  With enough live rows it is split: this call enqueues the probe (the front rows of all live
// slots, then k_probe_split) and pool_launch_drafts follows once the probe has published its match count.
static int pool_launch_step(PoolJob& j, int n_live) {
  ttx_session* s = j.s;
  StepCtx k = j.g.k;
  const int kcap = k.max_len;
  const long long rows = (long long)n_live * step_rps(k.N, k.D);
  if (!j.two_phase || rows < j.min_rows) {
    k.variant = variant_for_rows(s, rows, true);     // free choice: identical bits
    TTX_TRY(graph_replay(s, j.st, s->step_graphs, pool_key(j, k, k.variant, 0), [&]() -> int {
      TTX_TRY(launch_prefix_drafts(s, j.st, k));
      TTX_TRY(run_step(s, j.st, k, kcap));
      return launch_accept_and_commit(s, j.st, j.g, false);
    }));
    ++j.pool.launched;
    j.rows_executed += rows; j.unsplit_rows += rows;
    return TTX_OK;
  }
  DecState* st2 = s->state2.as<DecState>();          // [0] probe, [1] draft pass, then the executed-row count
  StepCtx kp = k;
  kp.N = 1; kp.D = 0; kp.sel_N = k.N; kp.sel_D = k.D;
  kp.st_ov = st2; kp.qkv_ov = s->qkv_probe.as<float>(); kp.pred_ov = s->pred_probe.as<int>();
  kp.variant = variant_for_rows(s, n_live, true);
  TTX_TRY(graph_replay(s, j.st, s->step_graphs, pool_key(j, k, kp.variant, j.draft_select ? 4 : 1), [&]() -> int {
    TTX_TRY(launch_prefix_drafts(s, j.st, k));       // before the probe: k_probe_split compares against the drafts
    hipLaunchKernelGGL(k_probe_begin, dim3(1), dim3(64), 0, j.st, s->state.as<DecState>(), st2);
    HIP_TRY(hipGetLastError());
    TTX_TRY(run_step(s, j.st, kp, kcap));
    ProbeSplitArgs ps{};
    ps.st = s->state.as<DecState>(); ps.act_idx = s->act_idx.as<int>(); ps.pred_probe = s->pred_probe.as<int>();
    ps.drafts = s->drafts.as<int>(); ps.N = k.N; ps.D = k.D; ps.act2 = s->act2.as<int>(); ps.pos2 = s->pos2.as<int>();
    ps.st2 = st2 + 1; ps.exec_rows = reinterpret_cast<int*>(st2 + 2);
    ps.host = j.dev_probe;
    if (j.draft_select) { ps.draft_mask = s->draft_mask.as<int>(); ps.row_base = s->row_base.as<int>(); ps.row_map = s->row_map.as<int>(); }
    hipLaunchKernelGGL(k_probe_split, dim3(1), dim3(k.B > 256 ? ACCEPT_THREADS : 256), 0, j.st, ps);
    HIP_TRY(hipGetLastError());
    return TTX_OK;
  }));
  ++j.probes;
  j.probe_pending = true;
  j.split_steps += 1; j.slot_steps += n_live; j.rows_executed += n_live;
  return TTX_OK;
}

// Second half of a split step, once the probe has published: the full step on the matching slots (skipped when there are none),
// then merge, accept and commit.
static int pool_launch_drafts(PoolJob& j) {
  ttx_session* s = j.s;
  StepCtx k = j.g.k;
  const int kcap = k.max_len;
  const int matches = ((volatile ProbeInfo*)s->probe_info)->matches;
  if (matches < 0 || matches > k.B) return fail(TTX_ERR_HIP, "slot pool: the probe published a match count outside the pool");
  const int RPS = step_rps(k.N, k.D);
  // rows of the draft pass: under draft select the compacted count the probe published, else every row of the matching slots
  const long long rows = j.draft_select ? ((volatile ProbeInfo*)s->probe_info)->rows : (long long)matches * RPS;
  if (rows < (long long)matches * (matches ? 1 + k.D : 0) || rows > (long long)matches * RPS)
    return fail(TTX_ERR_HIP, "slot pool: the probe published a row count outside its matches' rows");
  DecState* st2 = s->state2.as<DecState>();
  k.st_ov = st2 + 1; k.act_ov = s->act2.as<int>(); k.pred_ov = s->pred_draft.as<int>();
  if (j.draft_select) { k.row_base = s->row_base.as<int>(); k.draft_mask = s->draft_mask.as<int>(); k.row_map = s->row_map.as<int>(); }
  k.variant = matches ? variant_for_rows(s, rows, true) : 0;
  j.matched_slot_steps += matches; j.skipped_draft_passes += matches ? 0 : 1;
  j.rows_executed += rows; j.drafts_matched += (rows - matches) / k.D;
  const int phase = j.draft_select ? (matches ? 5 : 6) : (matches ? 2 : 3);
  TTX_TRY(graph_replay(s, j.st, s->step_graphs, pool_key(j, k, k.variant, phase), [&]() -> int {
    if (matches) TTX_TRY(run_step(s, j.st, k, kcap));
    MergePredArgs mp{};
    mp.st = s->state.as<DecState>(); mp.pos2 = s->pos2.as<int>(); mp.pred_probe = s->pred_probe.as<int>();
    mp.pred2 = s->pred_draft.as<int>(); mp.pred = s->pred.as<int>(); mp.RPS = RPS;
    mp.row_base = k.row_base; mp.draft_mask = k.draft_mask; mp.D = k.D;
    hipLaunchKernelGGL(k_merge_pred, dim3(cdiv(k.B * RPS, 256)), dim3(256), 0, j.st, mp);
    HIP_TRY(hipGetLastError());
    return launch_accept_and_commit(s, j.st, j.g2, false);
  }));
  j.probe_pending = false;
  ++j.pool.launched;
  return TTX_OK;
}

// After pool_start's allocations: the call's parameter block on the device; every step of the pool then draws with k_sample_step on
// the slots' keys and sample ids (written at admission) and accepts under the sampling rule.
static int pool_sample_begin(PoolJob& j, const SampleSetup& smp) {
  ttx_session* s = j.s;
  hipLaunchKernelGGL(k_sample_params, dim3(1), dim3(64), 0, j.st, s->smp_prm.as<SampleBlock>(), smp.blk);
  HIP_TRY(hipGetLastError());
  StepCtx& k = j.g.k;
  k.want_sample_step = true;
  k.sample.key = s->smp_key.as<unsigned long long>(); k.sample.sample = s->smp_sample.as<unsigned>();
  k.sample.front = s->front.as<int>(); k.sample.prm = s->smp_prm.as<SampleBlock>();
  j.g.la.sample_rule = 1;
  j.per_src = smp.n; j.d_row_keys = smp.d_row_keys;
  // every pool of the call holds the whole tables; a slot's prefix length, its rows of the tables and its draft 0 are written at
  // admission.  The class table is one for the call: nothing per slot, the state comes from the slot's row
  ConstraintTabs t;
  TTX_TRY(constraints_upload(s, j.st, smp, k.max_len, k.p.pad_token, s->pfx_len.as<int>(), s->pfx_src.as<int>(), s->lb_src.as<int>(), &t));
  k.bias = t.bias; k.syntax = t.syntax;
  if (smp.tabled()) {
    if (smp.proposed) { k.prop = t.pfx; k.prop_ctx = smp.prop_ctx; }
    else k.sample.pfx = t.pfx;
    k.pfx_draft0 = s->pfx_draft0.as<int>();
  }
  return TTX_OK;
}

// The two slot pools (arguments validated by the callers).  The work list holds R_total units of `per` decoder rows each, admitted
// together: the greedy pool's rows (per 1, smp null), the sampling pool's sources (per = num_samples).  d_src, h_len and the
// admission's length buckets go by unit; slots, d_out and the counters by decoder row.
static int pool_generate(ttx_session** sessions, int n_sessions, const int64_t* d_src, int R_total, int Ls_all, const int32_t* h_len,
                         int Ls_cap, int capacity, const ttx_gen_params* p, int64_t* d_out, int16_t* d_traj, int32_t* d_fin_step,
                         ttx_gen_stats* stats, void* stream, const SampleSetup* smp) {
  const int per = smp ? smp->n : 1;
  const PoolShape shape = pool_shape(n_sessions, R_total, R_total * per, capacity, 32, per);      // the work list: units
  const int n_jobs = shape.n_jobs, C = shape.C;
  std::vector<int> first(R_total + 1);
  for (int r = 0; r <= R_total; ++r) first[r] = r * per;
  PoolList list = pool_list(first.data(), R_total, n_jobs);
  std::vector<PoolJob> jobs(n_jobs);
  std::vector<int> chunk_ends;
  std::fill(std::begin(sessions[0]->pool_counters), std::end(sessions[0]->pool_counters), 0LL);
  // profiling sessions (bench.py's roofline pass): the pools run ONE AFTER ANOTHER, so that the event pair around a GEMM launch
  // measures that launch and not the kernels of three other pools sharing the device with it
  const bool serial = sessions[0]->profile;
  const long long max_launches = (long long)(p->max_len + 2) * (R_total + 1);
  const auto start = [&](int i) -> int {
    TTX_TRY(pool_start(jobs[i], sessions[i], sessions[i]->own_stream, C, Ls_cap, p, d_out, d_traj, d_fin_step, smp));
    // every pool of a call has the same model and reads the same environment: the mode is the call's
    if (i == 0) sessions[0]->pool_counters[6] = jobs[0].draft_select ? 1 : 0;
    return TTX_OK;
  };
  const auto turn = [&](int i) -> int {
    PoolJob& j = jobs[i];
    ttx_session* s = j.s;
    volatile HostInfo* hi = s->host_info;
    if (j.pool.phase == 1) {
      if (j.probe_pending) {
        if (((volatile ProbeInfo*)s->probe_info)->probes_done < j.probes) return TURN_WAITING;
        TTX_TRY(pool_launch_drafts(j));
        return TURN_PROGRESSED;
      }
      PoolLook look{hi->steps_done >= j.pool.launched, false, 0, 0};      // the error word is read with the counters, at collect time
      if (look.published) look.n_live = look.n_running = hi->n_active;
      const PoolPlan plan = pool_step(j.pool, list, look, i, C, serial, max_launches);
      switch (plan.act) {
        case PoolPlan::WAIT: return TURN_WAITING;
        case PoolPlan::FAILED:                        // not reached while look.error is false
          return fail(TTX_ERR_HIP, "slot pool bookkeeping failed (admitted more rows than free slots)");
        case PoolPlan::STUCK: return fail(TTX_ERR_HIP, "decode loop failed to terminate");
        case PoolPlan::DRAIN:
          TTX_TRY(enqueue_readback(s, j.st, s->state.p, sizeof(DecState)));
          j.pool.phase = 2;
          break;
        case PoolPlan::LAUNCH:
          if (plan.n_take > 0) {
            // every sub-chunk at the width of its own longest row; the staging buffers are the stream's, one sub-chunk after another
            admit_chunks(h_len + plan.first_batch, plan.n_take, j.admit_rows, chunk_ends);
            int r0 = plan.first_batch;
            for (const int end : chunk_ends) {
              const int r1 = plan.first_batch + end;
              TTX_TRY(pool_admit(j, d_src + (size_t)r0 * Ls_all, Ls_all, r1 - r0, chunk_width(h_len, r0, r1), r0, d_out, d_traj, d_fin_step));
              r0 = r1;
            }
          }
          TTX_TRY(pool_launch_step(j, plan.n_live));
          break;
      }
      return TURN_PROGRESSED;
    }
    if (hipEventQuery(s->ev_done) != hipSuccess) return TURN_IDLE;
    const DecState& hs = *s->host_state;
    if (stats) {
      add_counters(*stats, hs);
      stats->src_tokens_padded += j.src_tokens_padded;
      pool_finish(s, j.st, &stats->decode_ms);
    }
    if (getenv("TTX_TWO_PHASE_STATS"))
      fprintf(stderr, "[ttx two-phase] pool %d: %d steps, %lld split (%lld without a draft pass), %lld slot-steps probed, %lld matched, "
                      "%lld draft rows executed, %lld drafts matched\n",      // draft select off: N drafts per matching slot
              i, j.pool.launched, j.split_steps, j.skipped_draft_passes, j.slot_steps, j.matched_slot_steps,
              j.rows_executed - j.slot_steps - j.unsplit_rows, j.drafts_matched);
    long long* pc = sessions[0]->pool_counters;
    pc[0] += j.pool.launched; pc[1] += j.split_steps; pc[2] += j.slot_steps; pc[3] += j.matched_slot_steps;
    pc[4] += j.drafts_matched; pc[5] += j.rows_executed;
    j.pool.phase = 3;
    if (hs.error == 3) return fail(TTX_ERR_ROW_REPLAY, "a row emitted PAD inside its sequence: decode the batches as given");
    if (hs.error) return fail(TTX_ERR_HIP, "slot pool bookkeeping failed (admitted more rows than free slots)");
    return TURN_FINISHED;
  };
  const int rc = drive_sessions(sessions, n_jobs, serial, stream, start, turn);
  if (stats) stats->status = rc;
  return rc;
}

extern "C" int ttx_greedy_speculative_generate_pool(ttx_session** sessions, int n_sessions, const int64_t* d_src, int R_total,
                                                    int Ls_all, const int32_t* h_len, int capacity, const ttx_gen_params* p,
                                                    int64_t* d_out, int16_t* d_traj, int32_t* d_fin_step, ttx_gen_stats* stats,
                                                    void* stream) {
  if (!sessions || n_sessions <= 0 || !d_src || R_total < 0 || !h_len || capacity <= 0 || capacity > 4096 || !p || !d_out || !d_traj ||
      !d_fin_step)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_greedy_speculative_generate_pool");
  if (R_total == 0) return TTX_OK;
  if (p->max_len > 32000) return fail(TTX_ERR_INVALID, "max_len too large for the int16 trace");
  // the longest row fixes the slot width; rows are admitted in the order given (length-sorted lists pad least: a chunk
  // is encoded at the width of its longest row)
  int len_max = 0;
  for (int i = 0; i < R_total; ++i) len_max = std::max(len_max, (int)h_len[i]);
  if (len_max > Ls_all) return fail(TTX_ERR_INVALID, "row length beyond the source matrix width");
  const int Ls_cap = pool_slot_width(len_max, sessions[0]->m->cfg.max_positions);
  TTX_TRY(gen_validate(sessions[0], d_src, capacity, Ls_cap, p, d_out, false));
  return pool_generate(sessions, n_sessions, d_src, R_total, Ls_all, h_len, Ls_cap, capacity, p, d_out, d_traj, d_fin_step, stats, stream,
                       nullptr);
}

// ttx_sample_speculative_generate's rows over a whole list of sources on the slot pool: the n decoder rows of a source are admitted
// together, the step kernels are the pool's with the keyed draw where the argmax stands.
static int sample_speculative_generate_pool(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total, int Ls_all,
                                            const int32_t* h_len, const int64_t* d_row_keys, int capacity, const ttx_sample_spec_params* p,
                                            const ttx_sample_opts& o, const ttx_syntax* syn, int64_t* d_out, ttx_gen_stats* stats,
                                            void* stream) {
  const char* who = "ttx_sample_speculative_generate_pool";
  if (!sessions || n_sessions <= 0 || !d_src || S_total < 0 || !h_len || !p || !d_out)
    return fail(TTX_ERR_INVALID, std::string("bad argument to ") + who);
  for (int i = 0; i < n_sessions; ++i)
    if (!sessions[i]) return fail(TTX_ERR_INVALID, std::string("bad argument to ") + who);
  SampleSetup smp{};
  ttx_gen_params g{};
  TTX_TRY(sample_spec_validate(who, sessions[0], p, capacity, &smp, &g));
  if (capacity < p->sample.num_samples || capacity > 4096)
    return fail(TTX_ERR_INVALID, std::string(who) + ": capacity must lie in [num_samples, 4096]");
  int len_max = 0;
  for (int i = 0; i < S_total; ++i) len_max = std::max(len_max, (int)h_len[i]);
  if (len_max > Ls_all) return fail(TTX_ERR_INVALID, std::string(who) + ": source length beyond the source matrix width");
  const ttx_config& c = sessions[0]->m->cfg;
  const int Ls_cap = pool_slot_width(len_max, c.max_positions);
  if (Ls_cap > c.max_positions) return fail(TTX_ERR_INVALID, std::string(who) + ": slot width beyond the positional table");
  if (g.pad_token != c.pad_token) return fail(TTX_ERR_INVALID, std::string(who) + ": generator pad token differs from the model's");
  if (g.max_len + g.draft_len + 2 > c.max_positions) return fail(TTX_ERR_INVALID, std::string(who) + ": max_len + draft_len exceeds the positional table");
  TTX_TRY(constraints_validate(who, sessions[0], o, syn, S_total, g.max_len, &smp));
  if (S_total == 0) return TTX_OK;
  smp.d_row_keys = d_row_keys;
  return pool_generate(sessions, n_sessions, d_src, S_total, Ls_all, h_len, Ls_cap, capacity, &g, d_out, nullptr, nullptr, stats, stream, &smp);
}

extern "C" int ttx_sample_speculative_generate_pool(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total, int Ls_all,
                                                    const int32_t* h_len, const int64_t* d_row_keys, int capacity,
                                                    const ttx_sample_spec_params* p, int64_t* d_out, ttx_gen_stats* stats, void* stream) {
  return sample_speculative_generate_pool(sessions, n_sessions, d_src, S_total, Ls_all, h_len, d_row_keys, capacity, p, NO_OPTS, nullptr, d_out,
                                          stats, stream);
}

// The prompted pool: every pool of the call holds the whole prefix table; a slot gets its source's index and length at admission.
extern "C" int ttx_sample_speculative_generate_pool_prefix(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total,
                                                           int Ls_all, const int32_t* h_len, const int64_t* d_row_keys, int capacity,
                                                           const ttx_sample_spec_params* p, const int64_t* d_prefix, int ld_prefix,
                                                           const int32_t* h_prefix_len, int64_t* d_out, ttx_gen_stats* stats,
                                                           void* stream) {
  return sample_speculative_generate_pool(sessions, n_sessions, d_src, S_total, Ls_all, h_len, d_row_keys, capacity, p,
                                          opts_of(d_prefix, ld_prefix, h_prefix_len, nullptr, 0, nullptr), nullptr, d_out, stats, stream);
}

// The proposed pool: the proposal table rides through admission as the prefix table does.
extern "C" int ttx_sample_speculative_generate_pool_proposal(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total,
                                                             int Ls_all, const int32_t* h_len, const int64_t* d_row_keys, int capacity,
                                                             const ttx_sample_spec_params* p, const int64_t* d_prefix, int ld_prefix,
                                                             const int32_t* h_prefix_len, const int64_t* d_proposal, int ld_proposal,
                                                             const int32_t* h_proposal_len, int64_t* d_out, ttx_gen_stats* stats,
                                                             void* stream) {
  return sample_speculative_generate_pool(sessions, n_sessions, d_src, S_total, Ls_all, h_len, d_row_keys, capacity, p,
                                          opts_of(d_prefix, ld_prefix, h_prefix_len, d_proposal, ld_proposal, h_proposal_len), nullptr, d_out,
                                          stats, stream);
}

// The form that takes every option; the bias table is [S_total][ld_bias] in the order of d_src, and a slot gets its row at admission.
extern "C" int ttx_sample_speculative_generate_pool_ex(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total,
                                                       int Ls_all, const int32_t* h_len, const int64_t* d_row_keys, int capacity,
                                                       const ttx_sample_spec_params* p, const ttx_sample_opts* o, int64_t* d_out,
                                                       ttx_gen_stats* stats, void* stream) {
  return sample_speculative_generate_pool(sessions, n_sessions, d_src, S_total, Ls_all, h_len, d_row_keys, capacity, p, o ? *o : NO_OPTS,
                                          nullptr, d_out, stats, stream);
}

// The general form: ttx_sample_speculative_generate_pool_ex under a syntax constraint, one table for the call, nothing per slot.
extern "C" int ttx_sample_speculative_generate_pool_syntax(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total,
                                                           int Ls_all, const int32_t* h_len, const int64_t* d_row_keys, int capacity,
                                                           const ttx_sample_spec_params* p, const ttx_sample_opts* o,
                                                           const ttx_syntax* syntax, int64_t* d_out, ttx_gen_stats* stats, void* stream) {
  return sample_speculative_generate_pool(sessions, n_sessions, d_src, S_total, Ls_all, h_len, d_row_keys, capacity, p, o ? *o : NO_OPTS,
                                          syntax, d_out, stats, stream);
}

// Several batches in flight on one GPU: outputs per batch are identical to the one-at-a-time call.
static int generate_many_impl(ttx_session** sessions, int n_sessions, int n_batches, const int64_t* const* d_src, const int* B,
                              const int* Ls, const ttx_gen_params* p, int64_t* const* d_out, int16_t* const* d_traj,
                              int32_t* const* d_fin, ttx_gen_stats* stats, void* stream) {
  if (!sessions || n_sessions <= 0 || n_batches < 0 || !d_src || !B || !Ls || !p || !d_out)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_greedy_speculative_generate_many");
  if (d_traj)
    for (int i = 0; i < n_batches; ++i)
      if (!d_traj[i] || !d_fin || !d_fin[i]) return fail(TTX_ERR_INVALID, "missing trace buffer for a batch");
  for (int i = 0; i < n_batches; ++i) TTX_TRY(gen_validate(sessions[0], d_src[i], B[i], Ls[i], p, d_out[i], false));
  if (sessions[0]->profile) n_sessions = 1;      // profiling: one batch at a time, so that an event pair times its own launch
  return generate_batches(sessions, n_sessions, n_batches, d_src, B, Ls, p, d_out, d_traj, d_fin, stats, stream, false, nullptr);
}

extern "C" int ttx_greedy_speculative_generate_many(ttx_session** sessions, int n_sessions, int n_batches,
                                                    const int64_t* const* d_src, const int* B, const int* Ls,
                                                    const ttx_gen_params* p, int64_t* const* d_out, ttx_gen_stats* stats,
                                                    void* stream) {
  return generate_many_impl(sessions, n_sessions, n_batches, d_src, B, Ls, p, d_out, nullptr, nullptr, stats, stream);
}

// The same engine under the per-row width rule: rows neither wait for nor are cut short by the other rows of their
// device batch, and each row's front after every step is returned, so the caller may group rows by length and still
// reproduce, batch by batch, what the reference's loop does to the batches it was given (decoding.py replays it).
extern "C" int ttx_greedy_speculative_generate_rows(ttx_session** sessions, int n_sessions, int n_batches,
                                                    const int64_t* const* d_src, const int* B, const int* Ls,
                                                    const ttx_gen_params* p, int64_t* const* d_out, int16_t* const* d_traj,
                                                    int32_t* const* d_fin_step, ttx_gen_stats* stats, void* stream) {
  if (!d_traj || !d_fin_step) return fail(TTX_ERR_INVALID, "ttx_greedy_speculative_generate_rows needs the trace buffers");
  if (p && p->max_len > 32000) return fail(TTX_ERR_INVALID, "max_len too large for the int16 trace");
  return generate_many_impl(sessions, n_sessions, n_batches, d_src, B, Ls, p, d_out, d_traj, d_fin_step, stats, stream);
}

// ------------------------------------------------------------------------------------------------
// Beam-speculative bookkeeping
extern "C" int ttx_nucleus_mask(ttx_session* s, const float* d_logits, int rows, int V, float nucleus, int n_best, float fill,
                                float* d_out, void* stream) {
  if (!s || !d_logits || !d_out || rows < 0 || V <= 0) return fail(TTX_ERR_INVALID, "bad argument to ttx_nucleus_mask");
  if (V > 64 * NUC_VPL) return fail(TTX_ERR_INVALID, "ttx_nucleus_mask: vocabulary larger than 1024");
  if (n_best < 1 || n_best > NUC_MAX_KEEP) return fail(TTX_ERR_INVALID, "ttx_nucleus_mask: n_best must be in [1,32]");
  if (rows == 0) return TTX_OK;
  HIP_TRY(hipSetDevice(s->m->device));
  NucleusArgs a{d_logits, rows, V, nucleus, n_best, fill, d_out, nullptr, 0, nullptr};
  hipLaunchKernelGGL(k_nucleus, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

extern "C" int ttx_accepted_lengths(ttx_session* s, const float* d_logits, const int64_t* d_drafts, int R, int D, int V,
                                    float nucleus, int n_best, int32_t* d_n_ok, void* stream) {
  if (!s || !d_logits || !d_drafts || !d_n_ok || R < 0 || D <= 0 || V <= 0) return fail(TTX_ERR_INVALID, "bad argument to ttx_accepted_lengths");
  if (V > 64 * NUC_VPL) return fail(TTX_ERR_INVALID, "ttx_accepted_lengths: vocabulary larger than 1024");
  if (n_best < 1 || n_best > NUC_MAX_KEEP) return fail(TTX_ERR_INVALID, "ttx_accepted_lengths: n_best must be in [1,32]");
  if (R == 0) return TTX_OK;
  HIP_TRY(hipSetDevice(s->m->device));
  NucleusArgs a{d_logits, R, V, nucleus, n_best, 0.f, nullptr, d_drafts, D, d_n_ok};
  hipLaunchKernelGGL(k_nucleus, dim3(cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

extern "C" int ttx_ragged_topk(ttx_session* s, const float* d_score, const int32_t* d_offsets, int G, int max_group, int k,
                               float* d_top, int64_t* d_idx, void* stream) {
  if (!s || !d_score || !d_offsets || !d_top || !d_idx || G < 0 || k < 1 || max_group < 1)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_ragged_topk");
  if ((size_t)max_group * 4 > 150 * 1024) return fail(TTX_ERR_INVALID, "ttx_ragged_topk: group larger than the LDS image");
  if (G == 0) return TTX_OK;
  HIP_TRY(hipSetDevice(s->m->device));
  const size_t lds = (size_t)max_group * 4;
  TTX_TRY(raise_lds_limit(reinterpret_cast<const void*>(&k_ragged_topk), lds, s->attr_topk));
  RaggedTopkArgs a{d_score, d_offsets, k, d_top, d_idx};
  hipLaunchKernelGGL(k_ragged_topk, dim3(G), dim3(256), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Beam-search speculative decoding, whole loop native (speculative_decoding.py:428-598 all drafts, :600-845 smart drafts).
// Device kernels of one iteration: see "Native beam-speculative loop" in ttx_kernels.hip.h.  The host keeps the loop
// scalars of the reference (draft_len, width, num_of_empty_columns, postn_after_the_last_meaning_token, possible_draft_len)
// and learns {candidates holding EOS, longest new row, accepted-token marks} of every iteration from pinned words the
// last kernel of the iteration publishes — no stream synchronisation inside the loop.
struct BeamJob {
  ttx_session* s = nullptr;
  hipStream_t st = nullptr;
  ttx_beam_params p{};
  int B = 0, Ls = 0, K = 0, N = 0, D0 = 0, n_lib = 0, lib_ld = 0, max_cand = 0, gen_ld = 0, Lc = 0;
  bool smart = false;
  // loop scalars
  int n_cand = 0, beam = 1, dl = 0, width = 1, empty_cols = 0, after_last = 1, room = 0, prev_dl = 0, cur = 0;
  int launched = 0;
  int n_eos = 0;             // candidates holding EOS after the previous iteration (they are not decoded)
  int variant = GV_BIG;      // GemmVariant of the iteration about to be enqueued (from the live candidates; identical bits)
  int phase = 0;             // 0 idle, 1 iteration in flight, 2 finishing, 3 done
  bool any_iteration = false;
  ttx_beam_stats acc{};
  int64_t* d_out = nullptr;
  ttx_beam_stats* stats = nullptr;
  int rc = TTX_OK;
};

static int beam_validate(const ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_beam_params* p, const int64_t* d_out) {
  if (!s || !d_src || !p || !d_out || B <= 0 || Ls <= 1) return fail(TTX_ERR_INVALID, "bad argument to ttx_beam_speculative_generate");
  const ttx_config& c = s->m->cfg;
  if (p->n_best < 1 || p->n_best > NUC_MAX_KEEP) return fail(TTX_ERR_INVALID, "n_best must be in [1,32]");
  if (c.vocab_size > 64 * NUC_VPL) return fail(TTX_ERR_INVALID, "vocabulary larger than 1024");
  if (p->n_drafts <= 0) return fail(TTX_ERR_REFERENCE, "The number of drafts must be greater than 0");
  if (p->n_drafts > BS_MAX_SLOTS) return fail(TTX_ERR_INVALID, "n_drafts beyond the 64 draft slots of the bookkeeping kernels");
  if (p->pad_token == p->replace_token || p->eos_token == p->replace_token || p->eos_token == p->pad_token)
    return fail(TTX_ERR_REFERENCE, "pad, eos and replace tokens must be pairwise different");
  if (p->pad_token != c.pad_token) return fail(TTX_ERR_INVALID, "generator pad token differs from the model's");
  if (p->max_len < 3)          // possible_draft_len = max_len - 2 < 1: the reference's loop never runs and it returns an unbound name
    return fail(TTX_ERR_REFERENCE, "max_len < 3: the reference's loop body never runs (UnboundLocalError: new_candidates)");
  if (p->smart_drafts_mode && Ls - 5 <= 0) return fail(TTX_ERR_REFERENCE, "The number of drafts must be greater than 0");
  const int D = clamp_draft_len(p->draft_len, 5, 200);
  if (p->max_len + D + 3 > c.max_positions) return fail(TTX_ERR_INVALID, "max_len + draft_len exceeds the positional table");
  return TTX_OK;
}

static int beam_start(BeamJob& j, ttx_session* s, hipStream_t st, const int64_t* d_src, int B, int Ls, const ttx_beam_params* p,
                      int64_t* d_out, ttx_beam_stats* stats) {
  const ttx_model* m = s->m;
  const ttx_config& c = m->cfg;
  const int d = c.embedding_dim, Ld = c.num_decoder_layers;
  j = BeamJob{};
  j.s = s; j.st = st; j.p = *p; j.B = B; j.Ls = Ls; j.K = p->n_best; j.N = p->n_drafts; j.smart = p->smart_drafts_mode != 0;
  j.d_out = d_out; j.stats = stats;
  const int Dreq = clamp_draft_len(p->draft_len, 5, 200);            // :278-284
  // all drafts: make_drafts(src[:, 1:], draft_len, N, 5, 200) -> D0 = draft_len; smart: windows of draft_len + 1 tokens
  // (clamped again by make_drafts, drafting.py:48) whose first token is the key -> D0 = that - 1
  j.lib_ld = clamp_draft_len(Dreq + 1, 5, 200);
  j.D0 = j.smart ? j.lib_ld - 1 : Dreq;
  j.n_lib = Ls - 5;
  j.max_cand = B * j.K;
  j.gen_ld = p->max_len + j.D0 + 2;
  j.Lc = p->max_len + j.D0 + 2;
  const size_t MC = (size_t)j.max_cand;
  const size_t Mmax = MC * step_rps(j.N, j.D0);
  Needs need{st};
  need(s->tok_src, (size_t)B * Ls * 4); need(s->src_valid, (size_t)B * Ls); need(s->memory, (size_t)B * Ls * d * 4);
  need(s->memkv, (size_t)B * Ls * Ld * 2 * d * 4);
  need(s->drafts, MC * j.N * std::max(j.D0, 1) * 4);
  need(s->gen, MC * j.gen_ld * 4); need(s->front, MC * 4); need(s->act_idx, MC * 4);
  for (int i = 0; i < 2; ++i) { need(s->tk[i], (size_t)Ld * MC * j.Lc * d * 4); need(s->tv[i], (size_t)Ld * MC * j.Lc * d * 4); }
  need(s->t_prev_len, MC * 4); need(s->t_slot_of, MC * 4); need(s->t_src_of, MC * 4);
  need(s->bs_cand_next, MC * j.gen_ld * 8); need(s->bs_len_next, MC * 4); need(s->bs_fin_next, MC); need(s->bs_logp_next, MC * 4);
  need(s->bs_len, MC * 4); need(s->bs_fin, MC); need(s->bs_active, MC); need(s->bs_logp, MC * 4); need(s->bs_per_cand, MC * 4);
  need(s->bs_best_n, MC * 4); need(s->bs_best_slot, MC * 4); need(s->bs_chosen, MC * std::max(j.D0, 1) * 8);
  need(s->bs_hit, MC * (size_t)j.N * std::max(j.D0, 1));
  need(s->bs_parent, MC * 4); need(s->bs_parent_draft, MC * 4); need(s->bs_mark, MC * 4);
  need(s->bs_drafts_src, (size_t)B * (j.smart ? (size_t)j.n_lib * j.lib_ld : (size_t)j.N * j.D0) * 4);
  need(s->bs_cnt, sizeof(BeamCounters));
  const size_t dl1 = (size_t)j.D0 + 1;
  need(s->leaf_score, MC * dl1 * j.K * 4); need(s->leaf_tok, MC * dl1 * j.K * 4); need(s->leaf_cnt, MC * dl1 * 4);
  need(s->beam_summary, 8 * 4);
  need_step_workspaces(s, need, Mmax, (size_t)B * Ls);
  s->graphs_current();
  TTX_TRY(need.rc);
  if ((size_t)j.K * dl1 > 1023 || 2 * (size_t)j.K * dl1 * j.K * 4 > 150 * 1024)
    return fail(TTX_ERR_INVALID, "too many leaves per source for the selection kernel's LDS image");
  if (!s->beam_host) {
    if (hipHostMalloc((void**)&s->beam_host, sizeof(BeamHost), hipHostMallocMapped) != hipSuccess)
      return fail(TTX_ERR_NOMEM, "hipHostMalloc failed");
  }
  std::memset(s->beam_host, 0, sizeof(BeamHost));

  s->ev_used = 0;
  HIP_TRY(hipEventRecord(s->ev_a, st));
  // encoder + cross K/V once per source (:439 / :626); drafts (:430) or the draft library (:603-615)
  TTX_TRY(encode_sources(s, st, d_src, 0, B, Ls, s->src_valid.as<uint8_t>(), s->memkv.as<float>()));
  if (j.smart)
    TTX_TRY(launch_make_drafts<int>(st, s->tok_src.as<int>(), Ls, 0, B, Ls, j.n_lib, j.lib_ld, p->eos_token, p->pad_token,
                                    p->replace_token, s->bs_drafts_src.as<int>()));
  else
    TTX_TRY(launch_make_drafts<int>(st, s->tok_src.as<int>(), Ls, 1, B, Ls - 1, j.N, j.D0, p->eos_token, p->pad_token,
                                    p->replace_token, s->bs_drafts_src.as<int>()));
  hipLaunchKernelGGL(k_bs_init, dim3(64), dim3(256), 0, st, s->bs_cand_next.as<int64_t>(), j.gen_ld, s->bs_len_next.as<int>(),
                     s->bs_fin_next.as<uint8_t>(), s->bs_logp_next.as<float>(), s->bs_parent.as<int>(), s->bs_parent_draft.as<int>(),
                     j.max_cand, B, p->bos_token, p->pad_token, s->bs_cnt.as<BeamCounters>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev_b, st));
  // candidate c of an iteration belongs to source c / beam: the tree kernels read the map from t_src_of, filled per iteration
  j.n_cand = B; j.beam = 1; j.dl = j.D0; j.width = 1; j.empty_cols = 0; j.after_last = 1;
  j.room = p->max_len - j.after_last - 1;
  j.cur = 0; j.prev_dl = j.D0;
  j.phase = 1;
  return TTX_OK;
}

__global__ void k_bs_src_of(int* src_of, int n, int beam) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) src_of[i] = i / beam;
}

// ---- the pieces of one beam iteration, shared by the beam-speculative loop, its batch pool and standard beam search ----------
// k_bs_prep (the rows of the last selection -> this iteration's candidates and draft slots) and the candidate -> source map.
// `pa` arrives with the shape (ld, n_cand, beam, dl, N, pad) and, for the speculative loop, the draft-source fields set.
// Every enqueue_* helper below is two parts: it fills the kernel's argument struct from the session, and a launch_* function
// launches that struct (grid, block, dynamic LDS, VPL dispatch, raise_lds_limit).  The ttx_debug_* entries of the beam kernels
// call the launch_* part on the caller's operands, so a test launch is the production launch.
static int launch_bs_prep(hipStream_t st, int MC, const BeamPrepArgs& pa) {
  hipLaunchKernelGGL(k_bs_prep, dim3(MC), dim3(256), 0, st, pa);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int enqueue_bs_prep(ttx_session* s, hipStream_t st, int MC, BeamPrepArgs pa) {
  pa.cand_next = s->bs_cand_next.as<int64_t>(); pa.len_next = s->bs_len_next.as<int>();
  pa.fin_next = s->bs_fin_next.as<uint8_t>(); pa.logp_next = s->bs_logp_next.as<float>();
  pa.gen = s->gen.as<int>(); pa.front = s->front.as<int>(); pa.len = s->bs_len.as<int>(); pa.active = s->bs_active.as<uint8_t>();
  pa.finished = s->bs_fin.as<uint8_t>(); pa.logp = s->bs_logp.as<float>(); pa.per_cand = s->bs_per_cand.as<int>();
  pa.drafts32 = s->drafts.as<int>();
  TTX_TRY(launch_bs_prep(st, MC, pa));
  hipLaunchKernelGGL(k_bs_src_of, dim3(cdiv(MC, 256)), dim3(256), 0, st, s->t_src_of.as<int>(), MC, pa.beam);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// k_tree_cache: every candidate's KV cache in buffer `to` from its parent's in buffer `from` plus the rows the parent's accepted
// draft left in the previous step's Q/K/V buffer (layout (prev_N, prev_D)).  With slot maps (the batch pool: from == to) a
// candidate's cache lives in the slot the map names.
static int launch_tree_cache(hipStream_t st, int MC, int layers, const TreeCacheArgs& ca) {
  hipLaunchKernelGGL(k_tree_cache, dim3(MC, layers), dim3(256), 0, st, ca);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int enqueue_tree_cache(ttx_session* s, hipStream_t st, int MC, int Lc, int from, int to, const int* slot_parent,
                              const int* slot_self, int prev_N, int prev_D) {
  const int d = s->m->cfg.embedding_dim;
  TreeCacheArgs ca{};
  ca.len = s->bs_len.as<int>(); ca.parent = s->bs_parent.as<int>(); ca.parent_draft = s->bs_parent_draft.as<int>();
  ca.prev_len = s->t_prev_len.as<int>(); ca.active = s->bs_active.as<uint8_t>();
  ca.k_old = s->tk[from].as<float>(); ca.v_old = s->tv[from].as<float>();
  ca.k_new = s->tk[to].as<float>(); ca.v_new = s->tv[to].as<float>();
  ca.slot_parent = slot_parent; ca.slot_self = slot_self;
  ca.cache_seq_stride = (long long)Lc * d; ca.cache_layer_stride = (long long)MC * ca.cache_seq_stride;
  ca.qkv_prev = s->qkv.as<float>();
  ca.qkv_layer_stride = (long long)MC * step_rps(prev_N, prev_D) * 3 * d;
  ca.prev_slot_of = s->t_slot_of.as<int>(); ca.prev_N = prev_N; ca.prev_D = prev_D; ca.d = d;
  return launch_tree_cache(st, MC, s->m->cfg.num_decoder_layers, ca);
}

// k_bs_list: the running candidates -> the verify step's active list, slot map and DecState.
static int launch_bs_list(hipStream_t st, const BeamListArgs& la) {
  hipLaunchKernelGGL(k_bs_list, dim3(1), dim3(256), 0, st, la);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int enqueue_bs_list(ttx_session* s, hipStream_t st, int n_cand, int N, int dl) {
  BeamListArgs la{};
  la.active = s->bs_active.as<uint8_t>(); la.per_cand = s->bs_per_cand.as<int>(); la.len = s->bs_len.as<int>();
  la.n_cand = n_cand; la.N = N; la.dl = dl;
  la.act_idx = s->act_idx.as<int>(); la.slot_of = s->t_slot_of.as<int>(); la.prev_len = s->t_prev_len.as<int>();
  la.st = s->state.as<DecState>(); la.cnt = s->bs_cnt.as<BeamCounters>(); la.summary = s->beam_summary.as<int>();
  return launch_bs_list(st, la);
}

// The verify step of tree decoding: D + 1 new positions per (running candidate, draft slot) on the candidate's KV cache in
// buffer `cache`, logits only (the selection kernels read them).
static StepCtx tree_step_ctx(ttx_session* s, int MC, int Ls, int N, int D, int Lc, int gen_ld, int max_len, int cache, int variant) {
  StepCtx k{};
  k.B = MC; k.Ls = Ls; k.N = N; k.D = D; k.Lc = Lc; k.gen_ld = gen_ld; k.max_len = max_len;
  k.kcache = s->tk[cache].as<float>(); k.vcache = s->tv[cache].as<float>(); k.src_of = s->t_src_of.as<int>(); k.want_argmax = false;
  k.variant = variant;
  return k;
}

// k_bs_hits (which draft tokens the step's logits accept) and k_bs_leaves (the best draft per candidate and its leaves).
// `pool`: the batch pool's per-candidate draft lengths, live flags and batch maps (null: one batch, one draft length).
// `skip_hits_without_drafts`: the single-batch loop launches no k_bs_hits at dl == 0; the pool always launches it.
// `ha` / `le`: the launch of k_bs_hits / k_bs_leaves, null for none (both carry V, N and dl).  `vpl`: logits per lane the
// selection keeps in registers, 0 = the smallest of 4 / 8 / 16 that covers the vocabulary (same results), else that one.
static int launch_hits_leaves(hipStream_t st, int MC, const BeamHitsArgs* ha, const BeamLeaves2Args* le, int vpl) {
  const int V = ha ? ha->V : le->V, N = ha ? ha->N : le->N, dl = ha ? ha->dl : le->dl;
  const dim3 hits_grid(MC, cdiv(std::max(N * dl, 1), BS_HITS_WAVES));
  const size_t leaves_lds = (size_t)2 * (dl + 1) * 4;
  const auto launch = [&](auto v) {
    constexpr int VPL = decltype(v)::value;
    if (ha) hipLaunchKernelGGL(k_bs_hits<VPL>, hits_grid, dim3(BS_HITS_WAVES * 64), 0, st, *ha);
    if (le) hipLaunchKernelGGL(k_bs_leaves<VPL>, dim3(MC), dim3(BS_LEAVES_THREADS), leaves_lds, st, *le);
  };
  if (vpl == 0) vpl = V <= 256 ? 4 : (V <= 512 ? 8 : NUC_VPL);
  if (vpl == 4) launch(std::integral_constant<int, 4>{});
  else if (vpl == 8) launch(std::integral_constant<int, 8>{});
  else launch(std::integral_constant<int, NUC_VPL>{});
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int enqueue_hits_leaves(ttx_session* s, hipStream_t st, int MC, int n_cand, int N, int dl, int K, const ttx_beam_params& p,
                               bool smart, const BeamPoolArgs* pool, bool skip_hits_without_drafts) {
  const int V = s->m->cfg.vocab_size;
  BeamHitsArgs ha{};
  ha.logits = s->logits.as<float>(); ha.V = V; ha.finished = s->bs_fin.as<uint8_t>(); ha.slot_of = s->t_slot_of.as<int>();
  ha.per_cand = s->bs_per_cand.as<int>(); ha.drafts32 = s->drafts.as<int>();
  ha.n_cand = n_cand; ha.N = N; ha.dl = dl; ha.K = K; ha.nucleus = BS_NUCLEUS; ha.hit = s->bs_hit.as<uint8_t>();
  BeamLeaves2Args le{};
  le.logits = s->logits.as<float>(); le.V = V; le.finished = s->bs_fin.as<uint8_t>(); le.slot_of = s->t_slot_of.as<int>();
  le.per_cand = s->bs_per_cand.as<int>(); le.drafts32 = s->drafts.as<int>(); le.logp = s->bs_logp.as<float>();
  le.hit = s->bs_hit.as<uint8_t>(); le.cnt = s->bs_cnt.as<BeamCounters>();
  le.n_cand = n_cand; le.N = N; le.dl = dl; le.K = K; le.bos = p.bos_token; le.pad = p.pad_token; le.smart = smart ? 1 : 0;
  le.best_n = s->bs_best_n.as<int>(); le.best_slot = s->bs_best_slot.as<int>(); le.chosen = s->bs_chosen.as<int64_t>();
  le.leaf_score = s->leaf_score.as<float>(); le.leaf_tok = s->leaf_tok.as<int>(); le.leaf_cnt = s->leaf_cnt.as<int>();
  if (pool) {
    ha.dl_of = pool->cand_dl;
    le.live = pool->live; le.dl_of = pool->cand_dl; le.grp_of = pool->bat_grp; le.cand_batch = pool->cand_batch;
  }
  const bool hits = dl > 0 || !skip_hits_without_drafts;
  return launch_hits_leaves(st, MC, hits ? &ha : nullptr, &le, 0);
}

// The kernels of one iteration, in order, as a function of the job's scalars alone (so that the sequence can be captured
// once per shape and replayed).  `first`: no cache to derive (every candidate is a fresh <BOS> row); `cur`: which of the
// two cache buffers holds the parents' caches.
static int launch_beam_select(ttx_session* s, hipStream_t st, const BeamSelectArgs<int>& sa) {
  const size_t lds = 2 * (size_t)sa.beam * (sa.dl + 1) * sa.K * 4;
  TTX_TRY(raise_lds_limit(reinterpret_cast<const void*>(&k_beam_select<int>), lds, s->attr_select));
  hipLaunchKernelGGL(k_beam_select<int>, dim3(sa.B), dim3(256), lds, st, sa);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_beam_step(ttx_session* s, hipStream_t st, const BeamStepArgs& sa) {
  const size_t lds = (size_t)sa.beam * sa.V * 4;
  TTX_TRY(raise_lds_limit(reinterpret_cast<const void*>(&k_beam_step), lds, s->attr_step));
  hipLaunchKernelGGL(k_beam_step, dim3(sa.B), dim3(256), lds, st, sa);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// k_beam_step_masked with k_beam_step's launch shape (`pfx.tok` null: no forced prefixes).
static int launch_beam_step_masked(ttx_session* s, hipStream_t st, const BeamStepArgs& sa, const PrefixTab& pfx) {
  const size_t lds = (size_t)sa.beam * sa.V * 4;
  TTX_TRY(raise_lds_limit(reinterpret_cast<const void*>(&k_beam_step_masked), lds, s->attr_step_masked));
  hipLaunchKernelGGL(k_beam_step_masked, dim3(sa.B), dim3(256), lds, st, sa, pfx);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_sbs_step(ttx_session* s, hipStream_t st, const SbsStepArgs& sa) {
  const size_t lds = (size_t)sa.beam * sa.V * 4;
  TTX_TRY(raise_lds_limit(reinterpret_cast<const void*>(&k_sbs_step), lds, s->attr_sbs_step));
  hipLaunchKernelGGL(k_sbs_step, dim3(sa.B), dim3(256), lds, st, sa);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// The waves per source k_sbs_step_masked runs with: a wave owns whole parent rows, and a filtered row costs up to 32 dependent
// selection rounds, so wider beams get more waves (DESIGN.md §23 has the measurement).
static int sbs_masked_waves(int beam) { return beam <= 4 ? 4 : (beam <= 8 ? 8 : SBS_MASKED_MAX_WAVES); }

template <int VPL>
static int launch_sbs_step_masked_vpl(ttx_session* s, hipStream_t st, const SbsStepArgs& sa, int waves, bool& attr) {
  const size_t lds = (size_t)sa.beam * sa.V * 4;
  TTX_TRY(raise_lds_limit(reinterpret_cast<const void*>(&k_sbs_step_masked<VPL>), lds, attr));
  hipLaunchKernelGGL((k_sbs_step_masked<VPL>), dim3(sa.B), dim3(64 * waves), lds, st, sa);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// waves 0: production's choice.
static int launch_sbs_step_masked(ttx_session* s, hipStream_t st, const SbsStepArgs& sa, int waves = 0) {
  if (waves == 0) waves = sbs_masked_waves(sa.beam);
  if (sa.V <= 64) return launch_sbs_step_masked_vpl<1>(s, st, sa, waves, s->attr_sbs_step_masked[0]);
  if (sa.V <= 128) return launch_sbs_step_masked_vpl<2>(s, st, sa, waves, s->attr_sbs_step_masked[1]);
  if (sa.V <= 256) return launch_sbs_step_masked_vpl<4>(s, st, sa, waves, s->attr_sbs_step_masked[2]);
  if (sa.V <= 512) return launch_sbs_step_masked_vpl<8>(s, st, sa, waves, s->attr_sbs_step_masked[3]);
  return launch_sbs_step_masked_vpl<16>(s, st, sa, waves, s->attr_sbs_step_masked[4]);
}

static int beam_enqueue_iter(const BeamJob& j, bool first, int cur) {
  ttx_session* s = j.s;
  hipStream_t st = j.st;
  const int dl = j.dl, MC = j.max_cand;
  BeamPrepArgs pa{};
  pa.ld = j.gen_ld; pa.n_cand = j.n_cand; pa.beam = j.beam; pa.dl = dl; pa.N = j.N; pa.pad = j.p.pad_token;
  pa.smart = j.smart ? 1 : 0; pa.n_lib = j.n_lib; pa.lib_ld = j.lib_ld;
  pa.drafts_all = s->bs_drafts_src.as<int>(); pa.D0 = j.D0; pa.lib = s->bs_drafts_src.as<int>();
  TTX_TRY(enqueue_bs_prep(s, st, MC, pa));
  if (!first) TTX_TRY(enqueue_tree_cache(s, st, MC, j.Lc, cur, cur ^ 1, nullptr, nullptr, j.N, j.prev_dl));
  TTX_TRY(enqueue_bs_list(s, st, j.n_cand, j.N, dl));
  TTX_TRY(run_step(s, st, tree_step_ctx(s, MC, j.Ls, j.N, dl, j.Lc, j.gen_ld, j.p.max_len, cur ^ 1, j.variant),
                   key_capacity(j.width, j.p.max_len)));
  TTX_TRY(enqueue_hits_leaves(s, st, MC, j.n_cand, j.N, dl, j.K, j.p, j.smart, nullptr, true));
  BeamSelectArgs<int> sa{s->leaf_score.as<float>(), s->leaf_tok.as<int>(), s->leaf_cnt.as<int>(), s->gen.as<int>(), j.gen_ld, j.gen_ld,
                         j.gen_ld, s->bs_len.as<int>(), s->bs_chosen.as<int64_t>(), s->bs_best_slot.as<int>(), s->bs_fin.as<uint8_t>(),
                         j.B, j.beam, dl, j.K, j.p.pad_token, j.p.eos_token, s->bs_cand_next.as<int64_t>(), s->bs_logp_next.as<float>(),
                         s->bs_parent.as<int>(), s->bs_parent_draft.as<int>(), s->bs_mark.as<int>(), s->beam_summary.as<int>(),
                         s->bs_len_next.as<int>(), s->bs_fin_next.as<uint8_t>()};
  TTX_TRY(launch_beam_select(s, st, sa));
  BeamHost* dev_host = nullptr;
  HIP_TRY(hipHostGetDevicePointer((void**)&dev_host, (void*)s->beam_host, 0));
  hipLaunchKernelGGL(k_bs_publish, dim3(1), dim3(64), 0, st, s->beam_summary.as<int>(), dev_host, s->bs_cnt.as<BeamCounters>());
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// Enqueue one iteration (the loop condition of :464 / :652 was checked by the caller) through graph_replay, one graph per shape.
static int beam_launch_iter(BeamJob& j) {
  ttx_session* s = j.s;
  j.dl = std::min(j.room, j.dl);                                   // :476
  const int grow = j.dl + 1 - j.empty_cols;
  if (grow > 0) j.width += grow;
  const bool first = j.launched == 0;
  const int cur = j.cur;
  j.variant = variant_for_rows(s, (long long)std::max(1, j.n_cand - j.n_eos) * step_rps(j.N, j.dl), true);
  const GraphKey key{GS_BEAM_ITER, j.B, j.Ls, j.K, j.N, j.D0, j.smart ? 1 : 0, j.p.max_len, j.n_cand, j.beam, j.dl, j.prev_dl, cur,
                     key_capacity(j.width, j.p.max_len), first ? 1 : 0, j.p.pad_token, j.p.bos_token, j.p.eos_token, j.variant};
  TTX_TRY(graph_replay(s, j.st, s->iter_graphs, key, [&]() -> int { return beam_enqueue_iter(j, first, cur); }));
  ++j.launched;
  j.cur = cur ^ 1;
  j.prev_dl = j.dl;
  j.any_iteration = true;
  return TTX_OK;
}

// The published summary of the iteration just finished -> the reference's loop scalars (:578-598).  Returns true when the
// loop goes on.
static bool beam_after_iter(BeamJob& j) {
  const volatile int* sm = j.s->beam_host->summary;
  const int n_eos = sm[0], min_pad = sm[1], acc_sum = sm[2], acc_cnt = sm[3], err = sm[4];
  if (err) {
    j.rc = fail(TTX_ERR_REFERENCE, "a source has fewer candidate leaves than n_best (the reference asserts here, speculative_decoding.py:195)");
    return false;
  }
  j.acc.accepted_tokens += acc_sum;
  j.acc.produced_non_pad_tokens += acc_sum + acc_cnt;
  j.n_cand = j.B * j.K;
  j.beam = j.K;
  j.n_eos = n_eos;
  if (n_eos == j.B * j.K) return false;                             // :586
  const int max_real = j.gen_ld - min_pad;                          // longest new row
  j.empty_cols = j.width - max_real;                                // min over rows of their PAD count (:592)
  j.after_last = j.width - j.empty_cols;
  j.room = j.p.max_len - j.after_last - 1;
  if (!(j.room >= 1 && j.after_last <= j.p.max_len)) return false;  // :464
  if (j.p.max_steps > 0 && j.launched >= j.p.max_steps) {
    j.rc = fail(TTX_ERR_MAX_STEPS, "beam-speculative loop exceeded max_steps (non-terminating input)");
    return false;
  }
  return true;
}

static int beam_finish_enqueue(BeamJob& j) {
  ttx_session* s = j.s;
  // new_candidates.reshape(b_size, n_best, -1): rows of the last selection, `width` columns
  if (j.width > j.p.max_len) return fail(TTX_ERR_HIP, "beam-speculative loop: result wider than max_len (internal error)");
  HIP_TRY(hipMemcpy2DAsync(j.d_out, (size_t)j.p.max_len * 8, s->bs_cand_next.p, (size_t)j.gen_ld * 8, (size_t)j.width * 8,
                           (size_t)j.B * j.K, hipMemcpyDeviceToDevice, j.st));
  TTX_TRY(enqueue_readback(s, j.st, s->bs_cnt.p, sizeof(BeamCounters)));
  j.phase = 2;
  return TTX_OK;
}

static void beam_collect(BeamJob& j) {
  add_counters(j.acc, *reinterpret_cast<const BeamCounters*>(j.s->host_state));    // beam_start zeroed them
  j.acc.src_tokens_padded = (int64_t)j.B * j.Ls;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, j.s->ev_a, j.s->ev_b) == hipSuccess) j.acc.encode_ms = ms;
  if (hipEventElapsedTime(&ms, j.s->ev_b, j.s->ev_c) == hipSuccess) j.acc.decode_ms = ms;
  collect_gemm_profile(j.s, j.st);
  j.acc.out_width = j.width;
  j.acc.status = j.rc;
  if (j.stats) *j.stats = j.acc;
  j.phase = 3;
}

static_assert(sizeof(BeamCounters) <= sizeof(DecState), "the pinned read-back buffer is sized for DecState");

extern "C" int ttx_beam_speculative_generate_many(ttx_session** sessions, int n_sessions, int n_batches, const int64_t* const* d_src,
                                                  const int* B, const int* Ls, const ttx_beam_params* p, int64_t* const* d_out,
                                                  ttx_beam_stats* stats, void* stream) {
  if (!sessions || n_sessions <= 0 || n_batches < 0 || !d_src || !B || !Ls || !p || !d_out || !stats)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_beam_speculative_generate_many");
  for (int i = 0; i < n_sessions; ++i) if (!sessions[i]) return fail(TTX_ERR_INVALID, "null session");
  for (int i = 0; i < n_batches; ++i) TTX_TRY(beam_validate(sessions[0], d_src[i], B[i], Ls[i], p, d_out[i]));
  if (n_batches == 0) return TTX_OK;
  if (sessions[0]->profile) n_sessions = 1;      // profiling: one batch at a time (see the greedy driver)
  const int n_jobs = std::min(n_sessions, n_batches);
  std::vector<BeamJob> jobs(n_jobs);
  int next = 0, rc_batch = TTX_OK;               // as in generate_batches
  const auto turn = [&](int i) -> int {
    BeamJob& j = jobs[i];
    ttx_session* s = sessions[i];
    if (j.phase == 0 || j.phase == 3) {
      if (next >= n_batches) return TURN_FINISHED;
      const int b = next++;
      TTX_TRY(beam_start(j, s, s->own_stream, d_src[b], B[b], Ls[b], p, d_out[b], &stats[b]));
      TTX_TRY(beam_launch_iter(j));                                 // max_len >= 3: the first iteration always runs
      return TURN_PROGRESSED;
    }
    if (j.phase == 1) {
      if (((volatile BeamHost*)s->beam_host)->steps_done < j.launched) return TURN_WAITING;   // the iteration in flight has not published yet
      TTX_TRY(beam_after_iter(j) ? beam_launch_iter(j) : beam_finish_enqueue(j));
      return TURN_PROGRESSED;
    }
    if (hipEventQuery(s->ev_done) != hipSuccess) return TURN_IDLE;
    beam_collect(j);
    if (rc_batch == TTX_OK) rc_batch = j.rc;
    return TURN_PROGRESSED;
  };
  const int rc = drive_sessions(sessions, n_jobs, false, stream, [](int) { return TTX_OK; }, turn);
  return rc != TTX_OK ? rc : rc_batch;      // what ended the call (a hang, a failed launch) before what a batch reported
}

extern "C" int ttx_beam_speculative_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_beam_params* p,
                                             int64_t* d_out, ttx_beam_stats* stats, void* stream) {
  ttx_beam_stats local{};
  const int64_t* srcs[1] = {d_src};
  int64_t* outs[1] = {d_out};
  ttx_session* ss[1] = {s};
  if (!s) return fail(TTX_ERR_INVALID, "null session");
  return ttx_beam_speculative_generate_many(ss, 1, 1, srcs, &B, &Ls, p, outs, stats ? stats : &local, stream);
}

// ------------------------------------------------------------------------------------------------
// Beam-speculative batch pool (kernels and the argument for exactness: "Beam-speculative BATCH POOL" in
// ttx_loop_kernels.hip.h).  Host side: one job per session, each a pool of C source slots fed with whole batches from the
// caller's work list; an iteration is one fixed launch sequence (captured once per cache parity and GEMM variant) over every
// live candidate of every batch in the pool.
struct BeamPoolJob {
  ttx_session* s = nullptr;
  hipStream_t st = nullptr;
  ttx_beam_params p{};
  int C = 0, K = 0, N = 0, D0 = 0, lib_ld = 0, Ls_cap = 0, gen_ld = 0, Lc = 0, MC = 0;
  bool smart = false;
  BeamPoolArgs a{};
  BeamPoolIo io{};
  PoolState pool;                   // launched: iterations enqueued (pool_step, ttx_admit.h)
  int cur = 0;
  long long src_tokens_padded = 0;
};

// What the beam pool and the stochastic beam pool start with: the session's pinned BeamPoolHost words (allocated once) zeroed and
// their device address in *dev_host, the GEMM event pairs rewound, the start of the pool's device time recorded.
static int pool_host_begin(ttx_session* s, hipStream_t st, BeamPoolHost** dev_host) {
  if (!s->bp_host && hipHostMalloc((void**)&s->bp_host, sizeof(BeamPoolHost), hipHostMallocMapped) != hipSuccess)
    return fail(TTX_ERR_NOMEM, "hipHostMalloc failed");
  std::memset(s->bp_host, 0, sizeof(BeamPoolHost));
  HIP_TRY(hipHostGetDevicePointer((void**)dev_host, (void*)s->bp_host, 0));
  s->ev_used = 0;
  HIP_TRY(hipEventRecord(s->ev_a, st));
  return TTX_OK;
}

// A look at those words for pool_step: the counts only once the iteration in flight has published.
static PoolLook pool_look(const volatile BeamPoolHost* bh, int launched) {
  if (bh->steps_done < launched) return {false, false, 0, 0};
  return {true, bh->error != 0, bh->n_live, bh->n_running};
}

// The pool's eight bookkeeping launches (bpool_start, bpool_admit, bpool_enqueue_iter; one at a time: ttx_debug_bsp).
static int launch_bsp_init(hipStream_t st, const BeamPoolArgs& a, int* src_of, int* cand_src_len) {
  hipLaunchKernelGGL(k_bsp_init, dim3(64), dim3(256), 0, st, a, src_of, cand_src_len);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_bsp_admit(hipStream_t st, const BeamPoolArgs& a, int* new_slot, int* cand_src_len, int R, int first_row) {
  hipLaunchKernelGGL(k_bsp_admit, dim3(1), dim3(1), 0, st, a, new_slot, cand_src_len, R, first_row);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// k_bsp_fill's operands: the pool's own arrays from `a`, the staged sources of one admission from the caller.
static BeamPoolFillArgs bsp_fill_args(const BeamPoolArgs& a, const int* new_slot, int R, int first_row, int Ls_new, const int* tok_new,
                                      uint8_t* src_valid, const uint8_t* valid_new, const int* drafts_new, float* memkv,
                                      const float* memkv_new, int kv_row) {
  BeamPoolFillArgs f{};
  f.new_slot = new_slot; f.R = R; f.first_row = first_row;
  f.C = a.C; f.K = a.K; f.N = a.N; f.D0 = a.D0; f.ld = a.ld; f.Ls_cap = a.Ls_cap; f.Ls_new = Ls_new; f.max_len = a.max_len;
  f.pad = a.pad; f.bos = a.bos;
  f.cand_next = a.cand_next; f.len_next = a.len_next; f.fin_next = a.fin_next; f.logp_next = a.logp_next; f.parent = a.parent;
  f.parent_draft = a.parent_draft;
  f.tok = const_cast<int*>(a.tok); f.tok_new = tok_new; f.src_valid = src_valid; f.valid_new = valid_new;
  f.drafts_all = const_cast<int*>(a.drafts_all); f.drafts_new = drafts_new;
  f.memkv = memkv; f.memkv_new = memkv_new; f.kv_row = kv_row; f.io = a.io;
  return f;
}

static int launch_bsp_fill(hipStream_t st, const BeamPoolFillArgs& f) {
  hipLaunchKernelGGL(k_bsp_fill, dim3(f.R, 1 + f.Ls_new), dim3(256), 0, st, f);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_bsp_prep(hipStream_t st, const BeamPoolArgs& a) {
  hipLaunchKernelGGL(k_bsp_prep, dim3(a.C * a.K), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static size_t bsp_select_lds(int K, int D0) { return 2 * (size_t)K * (D0 + 1) * K * 4; }

static int launch_bsp_select(ttx_session* s, hipStream_t st, const BeamPoolArgs& a) {
  const size_t lds = bsp_select_lds(a.K, a.D0);
  TTX_TRY(raise_lds_limit(reinterpret_cast<const void*>(&k_bsp_select), lds, s->attr_pool_select));
  hipLaunchKernelGGL(k_bsp_select, dim3(a.C), dim3(256), lds, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_bsp_batches(hipStream_t st, const BeamPoolArgs& a) {
  hipLaunchKernelGGL(k_bsp_batches, dim3(cdiv(a.C, 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_bsp_retire(hipStream_t st, const BeamPoolArgs& a) {
  hipLaunchKernelGGL(k_bsp_retire, dim3(a.C), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_bsp_publish(hipStream_t st, const BeamPoolArgs& a) {
  hipLaunchKernelGGL(k_bsp_publish, dim3(cdiv(a.C, 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int bpool_start(BeamPoolJob& j, ttx_session* s, hipStream_t st, int C, int Ls_cap, const ttx_beam_params* p, const BeamPoolIo& io_host,
                       const int32_t* h_len, const int32_t* h_batch_of, const int32_t* h_given, int R_total, int n_batches) {
  const ttx_config& c = s->m->cfg;
  const int d = c.embedding_dim, Ld = c.num_decoder_layers;
  j = BeamPoolJob{};
  j.s = s; j.st = st; j.p = *p; j.C = C; j.K = p->n_best; j.N = p->n_drafts; j.smart = p->smart_drafts_mode != 0; j.Ls_cap = Ls_cap;
  const int Dreq = clamp_draft_len(p->draft_len, 5, 200);
  j.lib_ld = clamp_draft_len(Dreq + 1, 5, 200);
  j.D0 = j.smart ? j.lib_ld - 1 : Dreq;
  j.gen_ld = p->max_len + j.D0 + 2;
  j.Lc = p->max_len + j.D0 + 2;
  j.MC = C * j.K;
  const size_t MC = (size_t)j.MC;
  const size_t Mmax = MC * step_rps(j.N, j.D0);
  Needs need{st};
  need_source_slots(s, need, C, Ls_cap);
  need(s->bp_tok, (size_t)C * Ls_cap * 4);
  need(s->bp_enc_qkv, (size_t)C * Ls_cap * 3 * d * 4);      // admissions must not touch the step's Q/K/V rows (see run_encoder)
  need(s->drafts_new, (size_t)C * j.N * j.D0 * 4); need(s->bs_drafts_src, (size_t)C * j.N * j.D0 * 4);
  need(s->drafts, MC * j.N * j.D0 * 4);
  need(s->gen, MC * j.gen_ld * 4); need(s->front, MC * 4); need(s->act_idx, MC * 4);
  need(s->tk[0], (size_t)Ld * MC * j.Lc * d * 4); need(s->tv[0], (size_t)Ld * MC * j.Lc * d * 4);      // one buffer: candidate -> slot map
  need(s->t_prev_len, MC * 4); need(s->t_slot_of, MC * 4); need(s->t_src_of, MC * 4); need(s->bp_cand_len, MC * 4);
  need(s->bs_cand_next, MC * j.gen_ld * 8); need(s->bs_len_next, MC * 4); need(s->bs_fin_next, MC); need(s->bs_logp_next, MC * 4);
  need(s->bs_len, MC * 4); need(s->bs_fin, MC); need(s->bs_active, MC); need(s->bs_logp, MC * 4); need(s->bs_per_cand, MC * 4);
  need(s->bs_best_n, MC * 4); need(s->bs_best_slot, MC * 4); need(s->bs_chosen, MC * j.D0 * 8);
  need(s->bs_hit, MC * (size_t)j.N * j.D0); need(s->bs_mark, MC);            // bs_mark: the live flags of the pool
  need(s->bs_parent, MC * 4); need(s->bs_parent_draft, MC * 4); need(s->bp_cand, MC * 16);     // cand_dl, cand_batch, cache_slot, cache_slot_parent
  need(s->bs_cnt, sizeof(BeamCounters));
  const size_t dl1 = (size_t)j.D0 + 1;
  need(s->leaf_score, MC * dl1 * j.K * 4); need(s->leaf_tok, MC * dl1 * j.K * 4); need(s->leaf_cnt, MC * dl1 * 4);
  need(s->beam_summary, 8 * 4); need(s->bp_grp, 4 * 4);
  need(s->bp_row_of, (size_t)C * 4 * 3);                        // row_of, slot_batch, src_state
  need(s->bp_batch, (size_t)C * 4 * 10);                        // ten per-batch-slot arrays
  need(s->bp_src_acc, (size_t)C * 32);
  need(s->bp_new_slot, (size_t)C * 4);
  need(s->bp_io, sizeof(BeamPoolIo) + ((size_t)R_total * 2 + n_batches) * 4);
  need_step_workspaces(s, need, Mmax, (size_t)C * Ls_cap);
  s->graphs_current();
  TTX_TRY(need.rc);
  if ((size_t)j.K * dl1 > 1023 || 2 * (size_t)j.K * dl1 * j.K * 4 > 150 * 1024)
    return fail(TTX_ERR_INVALID, "too many leaves per source for the selection kernel's LDS image");
  BeamPoolHost* dev_host = nullptr;
  TTX_TRY(pool_host_begin(s, st, &dev_host));
  // the caller-side pointer block and the work list's lengths live in one device allocation:
  // [BeamPoolIo][len_all: R_total][batch_all: R_total][given_all: n_batches]
  char* io_dev = s->bp_io.as<char>();
  int* len_dev = reinterpret_cast<int*>(io_dev + sizeof(BeamPoolIo));
  int* batch_dev = len_dev + R_total;
  int* given_dev = batch_dev + R_total;
  j.io = io_host;
  j.io.len_all = len_dev; j.io.batch_all = batch_dev; j.io.given_all = given_dev;
  HIP_TRY(hipMemcpyAsync(io_dev, &j.io, sizeof(BeamPoolIo), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(len_dev, h_len, (size_t)R_total * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(batch_dev, h_batch_of, (size_t)R_total * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(given_dev, h_given, (size_t)n_batches * 4, hipMemcpyHostToDevice, st));
  BeamPoolArgs& a = j.a;
  a.C = C; a.K = j.K; a.N = j.N; a.D0 = j.D0; a.Ls_cap = Ls_cap; a.max_len = p->max_len; a.ld = j.gen_ld;
  a.smart = j.smart ? 1 : 0; a.lib_ld = j.lib_ld; a.pad = p->pad_token; a.bos = p->bos_token; a.eos = p->eos_token; a.repl = p->replace_token;
  a.max_steps = p->max_steps;
  a.row_of = s->bp_row_of.as<int>(); a.slot_batch = a.row_of + C; a.src_state = a.row_of + 2 * C; a.src_acc = s->bp_src_acc.as<int>();
  {
    int* bb = s->bp_batch.as<int>();
    a.bat_id = bb; a.bat_iter = bb + C; a.bat_dl = bb + 2 * C; a.bat_grp = bb + 3 * C; a.bat_live = bb + 4 * C; a.bat_nfin = bb + 5 * C;
    a.bat_longest_fin = bb + 6 * C; a.bat_longest_cur = bb + 7 * C; a.bat_state = bb + 8 * C; a.bat_given = bb + 9 * C;
  }
  a.cand_dl = s->bp_cand.as<int>(); a.cand_batch = a.cand_dl + j.MC; a.cache_slot = a.cand_dl + 2 * j.MC; a.cache_slot_parent = a.cand_dl + 3 * j.MC;
  a.tok = s->bp_tok.as<int>(); a.drafts_all = s->bs_drafts_src.as<int>();
  a.cand_next = s->bs_cand_next.as<int64_t>(); a.len_next = s->bs_len_next.as<int>(); a.fin_next = s->bs_fin_next.as<uint8_t>();
  a.logp_next = s->bs_logp_next.as<float>(); a.parent = s->bs_parent.as<int>(); a.parent_draft = s->bs_parent_draft.as<int>();
  a.gen = s->gen.as<int>(); a.front = s->front.as<int>(); a.len = s->bs_len.as<int>(); a.active = s->bs_active.as<uint8_t>();
  a.finished = s->bs_fin.as<uint8_t>(); a.live = s->bs_mark.as<uint8_t>(); a.logp = s->bs_logp.as<float>(); a.per_cand = s->bs_per_cand.as<int>();
  a.drafts32 = s->drafts.as<int>();
  a.chosen_slot = s->bs_best_slot.as<int>(); a.chosen = s->bs_chosen.as<int64_t>();
  a.leaf_score = s->leaf_score.as<float>(); a.leaf_tok = s->leaf_tok.as<int>(); a.leaf_cnt = s->leaf_cnt.as<int>();
  a.cnt = s->bs_cnt.as<BeamCounters>(); a.io = reinterpret_cast<const BeamPoolIo*>(io_dev); a.host = dev_host; a.dev_summary = s->bp_grp.as<int>();
  TTX_TRY(launch_bsp_init(st, a, s->t_src_of.as<int>(), s->bp_cand_len.as<int>()));
  HIP_TRY(hipEventRecord(s->ev_b, st));
  j.pool.phase = 1;
  return TTX_OK;
}

// Encode R new sources (rows first_row .. of the caller's matrix, Ls_new columns of it) and hand them free source slots.
static int bpool_admit(BeamPoolJob& j, const int64_t* d_src_rows, int ld_src, int R, int Ls_new, int first_row) {
  ttx_session* s = j.s;
  hipStream_t st = j.st;
  const int kv_row = s->m->cfg.num_decoder_layers * 2 * s->m->cfg.embedding_dim;
  TTX_TRY(encode_sources(s, st, d_src_rows, ld_src, R, Ls_new, s->valid_new.as<uint8_t>(), s->memkv_new.as<float>(), s->bp_enc_qkv.as<float>()));
  if (!j.smart)      // make_drafts(src[:, 1:], draft_len, N, 5, 200) (:430): independent of how far the row is padded
    TTX_TRY(launch_make_drafts<int>(st, s->tok_src.as<int>(), Ls_new, 1, R, Ls_new - 1, j.N, j.D0, j.p.eos_token, j.p.pad_token,
                                    j.p.replace_token, s->drafts_new.as<int>()));
  TTX_TRY(launch_bsp_admit(st, j.a, s->bp_new_slot.as<int>(), s->bp_cand_len.as<int>(), R, first_row));
  TTX_TRY(launch_bsp_fill(st, bsp_fill_args(j.a, s->bp_new_slot.as<int>(), R, first_row, Ls_new, s->tok_src.as<int>(), s->src_valid.as<uint8_t>(),
                                            s->valid_new.as<uint8_t>(), j.smart ? nullptr : s->drafts_new.as<int>(), s->memkv.as<float>(),
                                            s->memkv_new.as<float>(), kv_row)));
  j.src_tokens_padded += (long long)R * Ls_new;
  return TTX_OK;
}

static int bpool_enqueue_iter(const BeamPoolJob& j, int variant) {
  ttx_session* s = j.s;
  hipStream_t st = j.st;
  const int dl = j.D0, MC = j.MC;
  TTX_TRY(launch_bsp_prep(st, j.a));
  // ONE cache buffer and a candidate -> slot map (k_bsp_select): most children append in their parent's slot, few copy; fresh
  // candidates (parent -1) have nothing to inherit
  TTX_TRY(enqueue_tree_cache(s, st, MC, j.Lc, 0, 0, j.a.cache_slot_parent, j.a.cache_slot, j.N, dl));
  TTX_TRY(enqueue_bs_list(s, st, MC, j.N, dl));
  StepCtx k = tree_step_ctx(s, MC, j.Ls_cap, j.N, dl, j.Lc, j.gen_ld, j.p.max_len, 0, variant);
  k.cache_slot = j.a.cache_slot; k.src_len = s->bp_cand_len.as<int>();
  TTX_TRY(run_step(s, st, k, key_capacity(j.p.max_len, j.p.max_len)));
  TTX_TRY(enqueue_hits_leaves(s, st, MC, MC, j.N, dl, j.K, j.p, j.smart, &j.a, false));
  TTX_TRY(launch_bsp_select(s, st, j.a));
  TTX_TRY(launch_bsp_batches(st, j.a));
  TTX_TRY(launch_bsp_retire(st, j.a));
  TTX_TRY(launch_bsp_publish(st, j.a));
  return TTX_OK;
}

static int bpool_launch_iter(BeamPoolJob& j, int n_running) {
  ttx_session* s = j.s;
  const int variant = variant_for_rows(s, (long long)std::max(1, n_running) * step_rps(j.N, j.D0), true);
  const GraphKey key{GS_BEAM_POOL_ITER, j.C, j.Ls_cap, j.K, j.N, j.D0, j.smart ? 1 : 0, j.p.max_len, j.cur, variant, j.p.pad_token,
                     j.p.bos_token, j.p.eos_token, j.p.replace_token, j.p.max_steps};
  TTX_TRY(graph_replay(s, j.st, s->iter_graphs, key, [&]() -> int { return bpool_enqueue_iter(j, variant); }));
  ++j.pool.launched;
  j.cur ^= 1;
  return TTX_OK;
}

extern "C" int ttx_beam_speculative_generate_pool(ttx_session** sessions, int n_sessions, const int64_t* d_src, int R_total, int Ls_all,
                                                  const int32_t* h_len, const int32_t* h_batch_of, int n_batches,
                                                  const int32_t* h_given_ls, int capacity, const ttx_beam_params* p, int64_t* d_out,
                                                  int16_t* d_trace_len, int32_t* d_summary, int trace_cap, ttx_beam_stats* stats,
                                                  void* stream) {
  if (!sessions || n_sessions <= 0 || !d_src || R_total < 0 || !h_len || !h_batch_of || n_batches < 0 || !h_given_ls || capacity <= 0 ||
      capacity > 1024 || !p || !d_out || !d_trace_len || !d_summary || trace_cap <= 0 || trace_cap > 32000 || !stats)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_beam_speculative_generate_pool");
  if (R_total == 0) return TTX_OK;
  for (int i = 0; i < n_sessions; ++i) if (!sessions[i]) return fail(TTX_ERR_INVALID, "null session");
  // the work list: whole batches, in order; batch b owns the sources [first[b], first[b + 1])
  std::vector<int> first(n_batches + 1, 0);
  int len_max = 2, max_batch = 0;
  for (int i = 0, b = -1; i < R_total; ++i) {
    if (h_batch_of[i] != b) {
      if (h_batch_of[i] != b + 1 || h_batch_of[i] >= n_batches) return fail(TTX_ERR_INVALID, "h_batch_of must number the batches 0, 1, ... in order");
      b = h_batch_of[i];
      first[b] = i;
    }
    first[b + 1] = i + 1;
    if (h_len[i] < 2 || h_len[i] > Ls_all) return fail(TTX_ERR_INVALID, "row length outside [2, width of the source matrix]");
    if (h_given_ls[b] < h_len[i]) return fail(TTX_ERR_INVALID, "a batch's given width is smaller than one of its sources");
    if (p->smart_drafts_mode && h_given_ls[b] - 5 <= 0) return fail(TTX_ERR_REFERENCE, "The number of drafts must be greater than 0");
    len_max = std::max(len_max, (int)h_len[i]);
  }
  if (R_total > 0 && h_batch_of[R_total - 1] != n_batches - 1) return fail(TTX_ERR_INVALID, "n_batches does not match h_batch_of");
  for (int b = 0; b < n_batches; ++b) max_batch = std::max(max_batch, first[b + 1] - first[b]);
  if (max_batch > capacity) return fail(TTX_ERR_INVALID, "a batch has more sources than the pool has slots");
  const int Ls_cap = pool_slot_width(len_max, sessions[0]->m->cfg.max_positions);
  TTX_TRY(beam_validate(sessions[0], d_src, 1, Ls_cap, p, d_out));
  const PoolShape shape = pool_shape(n_sessions, n_batches, R_total, capacity, 8, max_batch);
  const int n_jobs = shape.n_jobs, C = shape.C;
  BeamPoolIo io{};
  io.out = d_out; io.trace_len = d_trace_len; io.summary = d_summary; io.T_cap = trace_cap;
  PoolList list = pool_list(first.data(), n_batches, n_jobs);
  std::vector<BeamPoolJob> jobs(n_jobs);
  const bool serial = sessions[0]->profile;                    // profiling sessions: one pool after another (see the greedy pool)
  const long long max_launches = (long long)(trace_cap + 2) * (R_total + 1);
  const auto t_call = std::chrono::steady_clock::now();
  ttx_beam_stats acc{};
  const auto start = [&](int i) -> int {
    return bpool_start(jobs[i], sessions[i], sessions[i]->own_stream, C, Ls_cap, p, io, h_len, h_batch_of, h_given_ls, R_total, n_batches);
  };
  const auto turn = [&](int i) -> int {
    BeamPoolJob& j = jobs[i];
    ttx_session* s = j.s;
    if (j.pool.phase == 1) {
      const PoolPlan plan = pool_step(j.pool, list, pool_look(s->bp_host, j.pool.launched), i, C, serial, max_launches);
      switch (plan.act) {
        case PoolPlan::WAIT: return TURN_WAITING;
        case PoolPlan::FAILED: return fail(TTX_ERR_HIP, "batch pool bookkeeping failed (admitted more sources than free slots)");
        case PoolPlan::STUCK: return fail(TTX_ERR_HIP, "batch pool failed to terminate");
        case PoolPlan::DRAIN:
          TTX_TRY(enqueue_readback(s, j.st, s->bs_cnt.p, sizeof(BeamCounters)));
          j.pool.phase = 2;
          break;
        case PoolPlan::LAUNCH:
          if (plan.n_take > 0)
            TTX_TRY(bpool_admit(j, d_src + (size_t)plan.first_row * Ls_all, Ls_all, plan.rows,
                                chunk_width(h_len, plan.first_row, plan.first_row + plan.rows), plan.first_row));
          if (s->host_timing)
            fprintf(stderr, "[ttx pool %d] t=%.3f ms iteration %d: %d live sources, %d running candidates, next batch %d of %d\n", i,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(), j.pool.launched + 1,
                    plan.n_live, plan.n_running, list.cursor, n_batches);
          TTX_TRY(bpool_launch_iter(j, plan.n_running));
          break;
      }
      return TURN_PROGRESSED;
    }
    if (hipEventQuery(s->ev_done) != hipSuccess) return TURN_IDLE;
    add_counters(acc, *reinterpret_cast<const BeamCounters*>(s->host_state));
    acc.src_tokens_padded += j.src_tokens_padded;
    pool_finish(s, j.st, &acc.decode_ms);
    j.pool.phase = 3;
    return TURN_FINISHED;
  };
  acc.status = drive_sessions(sessions, n_jobs, serial, stream, start, turn);
  *stats = acc;
  return acc.status;
}

// ------------------------------------------------------------------------------------------------
// Standard beam search, whole loop native (standard_decoding.py:89-174): per-hypothesis KV cache (the tree kernels),
// the verify-step kernels with one row per running hypothesis, k_beam_step for log-softmax + top-beam + row assembly.
struct BeamSearchJob {
  ttx_session* s = nullptr;
  hipStream_t st = nullptr;
  ttx_beam_search_params p{};
  int B = 0, Ls = 0, K = 0, MC = 0, ld = 0, Lc = 0;
  BeamHost* dev_host = nullptr;    // device address of the session's pinned summary words
  int n_cand = 0, beam = 1, width = 1, cur = 0, launched = 0;   // loop scalars
  int n_eos = 0;             // hypotheses holding EOS after the previous iteration
  int phase = 0;             // 0 not started, 1 iteration in flight, 2 finishing
  int64_t* d_out = nullptr;
  // stochastic beam search (ttx_sbs_generate): the same loop with k_sbs_step as the step kernel.  phi rides bs_logp / bs_logp_next;
  // G is read from sbs_g or sbs_g_next by the parity of the iteration and written to the other.
  bool sbs = false;
  float inv_T = 1.f;
  unsigned long long seed = 0;
  const int64_t* row_keys = nullptr;
  float* d_logp = nullptr; float* d_gumbel = nullptr;
  ttx_sbs_trace trace{};
  // ttx_sbs_generate_ex with a filter on or a non-empty prefix: k_sbs_step_masked instead (masked false: k_sbs_step, launch for launch)
  bool masked = false;
  int top_k = 0; float top_p = 1.f;
  PrefixTab pfx{};
  LogitBiasTab bias{};       // ttx_sbs_generate_bias: the session's table, by candidate (t_src_of); val null: no bias, no launch
  // ttx_beam_generate_constrained under a bias, a syntax table or a non-empty prefix: k_beam_step_masked instead of k_beam_step
  // (constrained false: k_beam_step, launch for launch).  `bias` and `pfx` above are shared with the stochastic form.
  bool constrained = false;
  const signed char* syntax = nullptr;   // the session's class table (syn_cls); null: no mask, no launch
  float* d_score = nullptr;              // [B, K] or null: the rows' cumulative scores
};

// Everything of the call behind the argument check: the reference's asserts and this library's limits, the workspaces, the
// encoder and the <BOS> hypotheses.
static int bsearch_start(BeamSearchJob& j, ttx_session* s, hipStream_t st, const int64_t* d_src, int B, int Ls,
                         const ttx_beam_search_params* p, int64_t* d_out, bool sbs) {
  const ttx_config& c = s->m->cfg;
  const int K = p->beam_size, max_len = p->max_len, V = c.vocab_size;
  if (max_len <= 1) return fail(TTX_ERR_REFERENCE, "assert self.max_len > 1 (standard_decoding.py:79)");
  if (K <= 0) return fail(TTX_ERR_REFERENCE, "assert self.beam_size > 0 (standard_decoding.py:80)");
  if (K > V) return fail(TTX_ERR_REFERENCE, "beam_size larger than the vocabulary: topk(k) of the first step raises");
  if ((size_t)K * V * 4 > 150 * 1024) return fail(TTX_ERR_INVALID, "beam_size x vocabulary beyond the selection kernel's LDS image");
  if (p->pad_token != c.pad_token) return fail(TTX_ERR_INVALID, "generator pad token differs from the model's");
  if (max_len + 2 > c.max_positions) return fail(TTX_ERR_INVALID, "max_len exceeds the positional table");
  j = BeamSearchJob{};
  j.s = s; j.st = st; j.p = *p; j.B = B; j.Ls = Ls; j.K = K; j.d_out = d_out; j.sbs = sbs;
  s->ev_used = 0;                     // profiling sessions: the event pairs of this call start from the first one
  const int d = c.embedding_dim, Ld = c.num_decoder_layers;
  const int MC = B * K, ld = max_len + 2, Lc = max_len + 2;
  const size_t Mmax = (size_t)MC;
  Needs need{st};
  need(s->tok_src, (size_t)B * Ls * 4); need(s->src_valid, (size_t)B * Ls); need(s->memory, (size_t)B * Ls * d * 4);
  need(s->memkv, (size_t)B * Ls * Ld * 2 * d * 4);
  need(s->drafts, (size_t)MC * 4);
  need(s->gen, (size_t)MC * ld * 4); need(s->front, (size_t)MC * 4); need(s->act_idx, (size_t)MC * 4);
  for (int i = 0; i < 2; ++i) { need(s->tk[i], (size_t)Ld * MC * Lc * d * 4); need(s->tv[i], (size_t)Ld * MC * Lc * d * 4); }
  need(s->t_prev_len, (size_t)MC * 4); need(s->t_slot_of, (size_t)MC * 4); need(s->t_src_of, (size_t)MC * 4);
  need(s->bs_cand_next, (size_t)MC * ld * 8); need(s->bs_len_next, (size_t)MC * 4); need(s->bs_fin_next, (size_t)MC);
  need(s->bs_logp_next, (size_t)MC * 4); need(s->bs_len, (size_t)MC * 4); need(s->bs_fin, (size_t)MC); need(s->bs_active, (size_t)MC);
  need(s->bs_logp, (size_t)MC * 4); need(s->bs_per_cand, (size_t)MC * 4); need(s->bs_parent, (size_t)MC * 4);
  need(s->bs_parent_draft, (size_t)MC * 4); need(s->bs_cnt, sizeof(BeamCounters)); need(s->beam_summary, 8 * 4);
  if (sbs) { need(s->sbs_g, (size_t)MC * 4); need(s->sbs_g_next, (size_t)MC * 4); }
  need_step_workspaces(s, need, Mmax, (size_t)B * Ls);
  s->graphs_current();
  TTX_TRY(need.rc);
  if (!s->beam_host && hipHostMalloc((void**)&s->beam_host, sizeof(BeamHost), hipHostMallocMapped) != hipSuccess)
    return fail(TTX_ERR_NOMEM, "hipHostMalloc failed");
  std::memset(s->beam_host, 0, sizeof(BeamHost));
  HIP_TRY(hipHostGetDevicePointer((void**)&j.dev_host, (void*)s->beam_host, 0));
  if (sbs) HIP_TRY(hipMemsetAsync(s->sbs_g.p, 0, (size_t)MC * 4, st));       // G = 0 for the <BOS> candidates
  // self.model(src, y) of the first step = encoder + the decoder on <BOS>; the reference then re-encodes the source once per
  // beam (:120-124): identical rows, so the beams of a source share its memory row here
  TTX_TRY(encode_sources(s, st, d_src, 0, B, Ls, s->src_valid.as<uint8_t>(), s->memkv.as<float>()));
  hipLaunchKernelGGL(k_bs_init, dim3(64), dim3(256), 0, st, s->bs_cand_next.as<int64_t>(), ld, s->bs_len_next.as<int>(),
                     s->bs_fin_next.as<uint8_t>(), s->bs_logp_next.as<float>(), s->bs_parent.as<int>(), s->bs_parent_draft.as<int>(),
                     MC, B, p->bos_token, p->pad_token, s->bs_cnt.as<BeamCounters>());
  HIP_TRY(hipGetLastError());
  j.MC = MC; j.ld = ld; j.Lc = Lc; j.n_cand = B; j.phase = 1;
  return TTX_OK;
}

// Enqueue one iteration.  width changes every step, so a step's graph would be replayed once: the steps run eagerly (about 12
// launches per decoder layer, enqueued well ahead of the device).
static int bsearch_launch_iter(BeamSearchJob& j) {
  ttx_session* s = j.s;
  hipStream_t st = j.st;
  const int max_len = j.p.max_len, cur = j.cur;
  BeamPrepArgs pa{};
  pa.ld = j.ld; pa.n_cand = j.n_cand; pa.beam = j.beam; pa.dl = 0; pa.N = 1; pa.pad = j.p.pad_token; pa.smart = 0;
  TTX_TRY(enqueue_bs_prep(s, st, j.MC, pa));
  if (j.launched > 0) TTX_TRY(enqueue_tree_cache(s, st, j.MC, j.Lc, cur, cur ^ 1, nullptr, nullptr, 1, 0));
  TTX_TRY(enqueue_bs_list(s, st, j.n_cand, 1, 0));
  const int variant = variant_for_rows(s, (long long)std::max(1, j.n_cand - j.n_eos), true);
  StepCtx k = tree_step_ctx(s, j.MC, j.Ls, 1, 0, j.Lc, j.ld, max_len, cur ^ 1, variant);
  k.bias = j.bias;                 // the step kernels below then read biased logits
  k.syntax = j.syntax;             // and masked ones: gen, front = len - 1 (k_bs_prep) and act_idx (k_bs_list) are what the mask's
  k.p.eos_token = j.p.eos_token;   // step mapping reads at (N, D) = (1, 0); the rule's EOS and max_len are the call's
  TTX_TRY(run_step(s, st, k, key_capacity(j.width, max_len)));
  if (j.sbs) {
    SbsStepArgs sa{};
    float* const gbuf[2] = {s->sbs_g.as<float>(), s->sbs_g_next.as<float>()};
    sa.logits = s->logits.as<float>(); sa.V = s->m->cfg.vocab_size; sa.slot_of = s->t_slot_of.as<int>(); sa.finished = s->bs_fin.as<uint8_t>();
    sa.phi = s->bs_logp.as<float>(); sa.g = gbuf[j.launched & 1]; sa.gen = s->gen.as<int>(); sa.ld = j.ld; sa.width = j.width;
    sa.B = j.B; sa.beam = j.beam; sa.K = j.K; sa.pad = j.p.pad_token; sa.eos = j.p.eos_token;
    sa.row_keys = j.row_keys; sa.seed = j.seed; sa.pos = j.width; sa.inv_T = j.inv_T;
    sa.new_cand = s->bs_cand_next.as<int64_t>(); sa.new_phi = s->bs_logp_next.as<float>(); sa.new_g = gbuf[(j.launched & 1) ^ 1];
    sa.parent = s->bs_parent.as<int>(); sa.new_len = s->bs_len_next.as<int>(); sa.new_finished = s->bs_fin_next.as<uint8_t>();
    sa.parent_draft = s->bs_parent_draft.as<int>(); sa.summary = s->beam_summary.as<int>();
    if (j.trace.d_parent) {
      const size_t at = (size_t)j.launched * j.B * j.K;
      sa.tr_parent = j.trace.d_parent + at; sa.tr_token = j.trace.d_token + at; sa.tr_phi = j.trace.d_phi + at; sa.tr_g = j.trace.d_g + at;
    }
    if (j.masked) {
      sa.top_k = j.top_k; sa.top_p = j.top_p; sa.pfx = j.pfx;
      TTX_TRY(launch_sbs_step_masked(s, st, sa));
    } else {
      TTX_TRY(launch_sbs_step(s, st, sa));
    }
    hipLaunchKernelGGL(k_bs_publish, dim3(1), dim3(64), 0, st, s->beam_summary.as<int>(), j.dev_host, s->bs_cnt.as<BeamCounters>());
    HIP_TRY(hipGetLastError());
    ++j.launched;
    j.cur = cur ^ 1;
    return TTX_OK;
  }
  BeamStepArgs sa{};
  sa.logits = s->logits.as<float>(); sa.V = s->m->cfg.vocab_size; sa.slot_of = s->t_slot_of.as<int>(); sa.finished = s->bs_fin.as<uint8_t>();
  sa.score = s->bs_logp.as<float>(); sa.gen = s->gen.as<int>(); sa.ld = j.ld; sa.width = j.width;
  sa.B = j.B; sa.beam = j.beam; sa.K = j.K; sa.pad = j.p.pad_token; sa.eos = j.p.eos_token;
  sa.new_cand = s->bs_cand_next.as<int64_t>(); sa.new_score = s->bs_logp_next.as<float>(); sa.parent = s->bs_parent.as<int>();
  sa.new_len = s->bs_len_next.as<int>(); sa.new_finished = s->bs_fin_next.as<uint8_t>(); sa.parent_draft = s->bs_parent_draft.as<int>();
  sa.summary = s->beam_summary.as<int>();
  if (j.constrained) {
    TTX_TRY(launch_beam_step_masked(s, st, sa, j.pfx));
    s->beam_step_masked_launches += 1;
  } else {
    TTX_TRY(launch_beam_step(s, st, sa));
  }
  hipLaunchKernelGGL(k_bs_publish, dim3(1), dim3(64), 0, st, s->beam_summary.as<int>(), j.dev_host, s->bs_cnt.as<BeamCounters>());
  HIP_TRY(hipGetLastError());
  ++j.launched;
  j.cur = cur ^ 1;
  return TTX_OK;
}

// The published summary of the iteration just finished -> the loop scalars.  Returns true when the loop goes on: the <BOS> step
// plus `predictions - 1` loop iterations (:127-131).
static bool bsearch_after_iter(BeamSearchJob& j) {
  const bool first = j.launched == 1;
  j.width += 1;
  j.n_cand = j.B * j.K; j.beam = j.K;
  j.n_eos = ((volatile BeamHost*)j.s->beam_host)->summary[0];
  if (j.n_eos == j.B * j.K && (!first || j.sbs)) return false;   // :166 (the check sits inside the loop, after the first step; the
                                                                 // stochastic rule stops as soon as every candidate is finished)
  return j.launched < j.p.max_len - 1;
}

static int bsearch_finish_enqueue(BeamSearchJob& j) {
  ttx_session* s = j.s;
  // the rows are PAD beyond `width` up to their stride ld = max_len + 2: the stochastic form hands out all max_len columns
  HIP_TRY(hipMemcpy2DAsync(j.d_out, (size_t)j.p.max_len * 8, s->bs_cand_next.p, (size_t)j.ld * 8, (size_t)(j.sbs ? j.p.max_len : j.width) * 8,
                           (size_t)j.B * j.K, hipMemcpyDeviceToDevice, j.st));
  if (j.sbs) {
    const Buf& g = (j.launched & 1) ? s->sbs_g_next : s->sbs_g;
    if (j.d_logp) HIP_TRY(hipMemcpyAsync(j.d_logp, s->bs_logp_next.p, (size_t)j.B * j.K * 4, hipMemcpyDeviceToDevice, j.st));
    if (j.d_gumbel) HIP_TRY(hipMemcpyAsync(j.d_gumbel, g.p, (size_t)j.B * j.K * 4, hipMemcpyDeviceToDevice, j.st));
  }
  if (j.d_score) HIP_TRY(hipMemcpyAsync(j.d_score, s->bs_logp_next.p, (size_t)j.B * j.K * 4, hipMemcpyDeviceToDevice, j.st));
  TTX_TRY(enqueue_readback(s, j.st, s->bs_cnt.p, sizeof(BeamCounters)));
  j.phase = 2;
  return TTX_OK;
}

// The three single-session beam loops (standard, constrained, stochastic) under drive_sessions.  `start` sizes the call's buffers,
// runs bsearch_start, sets the job's options and enqueues the first iteration (max_len > 1: it always runs); a turn enqueues the
// next iteration, or the copies of the results, once the one in flight has published.
template <class Start>
static int bsearch_drive(BeamSearchJob& j, ttx_session* s, ttx_beam_search_stats* stats, void* stream, Start start) {
  const auto turn = [&](int) -> int {
    if (j.phase == 1) {
      if (((volatile BeamHost*)s->beam_host)->steps_done < j.launched) return TURN_WAITING;   // the iteration in flight has not published yet
      TTX_TRY(bsearch_after_iter(j) ? bsearch_launch_iter(j) : bsearch_finish_enqueue(j));
      return TURN_PROGRESSED;
    }
    if (hipEventQuery(s->ev_done) != hipSuccess) return TURN_IDLE;
    const BeamCounters* cn = reinterpret_cast<const BeamCounters*>(s->host_state);
    stats->model_calls = cn->model_calls; stats->running_rows = cn->running_cands; stats->out_width = j.width;
    return TURN_FINISHED;
  };
  return drive_sessions(&s, 1, false, stream, start, turn);
}

// Before bsearch_start settles which graphs are current: the buffers of a beam call's constraints.  Its tables go by source; the
// prefix table's row-to-source map is the identity over the B sources (k_sbs_prefix_src).
static int bsearch_constraints_ensure(ttx_session* s, hipStream_t st, const SampleSetup& c, int B, int max_len) {
  return constraints_ensure(s, st, c, max_len, 0, 0, c.prompted ? (size_t)B : 0);
}

// After bsearch_start: the call's tables into the job.  The bias goes by candidate (t_src_of); the steps run eagerly, yet read
// the session's copies as every constrained loop does.
static int bsearch_constraints_upload(BeamSearchJob& j, const SampleSetup& c) {
  ttx_session* s = j.s;
  ConstraintTabs t;
  TTX_TRY(constraints_upload(s, j.st, c, j.p.max_len, j.p.pad_token, s->pfx_len_src.as<int>(), s->smp_src_of.as<int>(), s->t_src_of.as<int>(), &t));
  j.bias = t.bias; j.syntax = t.syntax; j.pfx = t.pfx;
  if (c.prompted) {
    hipLaunchKernelGGL(k_sbs_prefix_src, dim3(cdiv(j.B, 256)), dim3(256), 0, j.st, s->smp_src_of.as<int>(), j.B);
    HIP_TRY(hipGetLastError());
  }
  return TTX_OK;
}

// Standard beam search and its constrained form: the beam loop above under a per-source logit bias (k_logit_bias), a syntax
// constraint (k_syntax_mask) and forced prefixes, with k_beam_step_masked (csrc/ttx_beam_mask.hip.h) where it launches k_beam_step.
// A call with none of the three is ttx_beam_generate, launch for launch; the copy of the scores hangs on d_score alone.
static int beam_generate(const char* who, ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_beam_search_params* p,
                         const ttx_sample_opts& o, const ttx_syntax* syntax, int64_t* d_out, float* d_score, ttx_beam_search_stats* stats,
                         void* stream) {
  if (!s || !d_src || !p || !d_out || !stats || B <= 0 || Ls <= 1) return fail(TTX_ERR_INVALID, std::string("bad argument to ") + who);
  SampleSetup c{};
  TTX_TRY(constraints_validate(who, s, o, syntax, B, p->max_len, &c));
  BeamSearchJob j;
  return bsearch_drive(j, s, stats, stream, [&](int) -> int {
    TTX_TRY(bsearch_constraints_ensure(s, s->own_stream, c, B, p->max_len));
    TTX_TRY(bsearch_start(j, s, s->own_stream, d_src, B, Ls, p, d_out, false));
    j.d_score = d_score;
    j.constrained = c.any();
    TTX_TRY(bsearch_constraints_upload(j, c));
    return bsearch_launch_iter(j);
  });
}

extern "C" int ttx_beam_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_beam_search_params* p, int64_t* d_out,
                                 ttx_beam_search_stats* stats, void* stream) {
  return beam_generate("ttx_beam_generate", s, d_src, B, Ls, p, NO_OPTS, nullptr, d_out, nullptr, stats, stream);
}

extern "C" int ttx_beam_generate_constrained(ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_beam_search_params* p,
                                             const float* d_bias, int ld_bias, const ttx_syntax* syntax, const int64_t* d_prefix,
                                             int ld_prefix, const int32_t* h_prefix_len, int64_t* d_out, float* d_score,
                                             ttx_beam_search_stats* stats, void* stream) {
  ttx_sample_opts o = opts_of(d_prefix, ld_prefix, h_prefix_len, nullptr, 0, nullptr);
  o.d_bias = d_bias; o.ld_bias = ld_bias;
  return beam_generate("ttx_beam_generate_constrained", s, d_src, B, Ls, p, o, syntax, d_out, d_score, stats, stream);
}

// The parameters and the filter of a stochastic beam search call over a model `cfg`, or TTX_ERR_INVALID: inv_T, and the filter as the
// step kernel takes it (a null `f` is none; a top_p alone runs as top_k = 32, as the sampler runs it).  `who.call` names the refusals
// of the parameters, `who.ex` those of the filter.
static int sbs_validate(const Who& who, const ttx_config& cfg, const ttx_sbs_params* p, const ttx_sbs_filter* f, float* inv_T, int* top_k,
                        float* top_p) {
  const std::string w = who.call, x = who.ex;
  const int V = cfg.vocab_size;
  if (p->max_len <= 1) return fail(TTX_ERR_INVALID, w + ": max_len must exceed 1");
  if (p->beam_size < 1 || p->beam_size > SBS_MAX_BEAM) return fail(TTX_ERR_INVALID, w + ": beam_size must lie in [1, 32]");
  if (V > SBS_MAX_V) return fail(TTX_ERR_INVALID, w + ": vocab_size above 1024");
  if (p->beam_size > V) return fail(TTX_ERR_INVALID, w + ": beam_size larger than the vocabulary");
  if (!(p->temperature > 0.0f) || !std::isfinite(p->temperature)) return fail(TTX_ERR_INVALID, w + ": temperature must be finite and > 0");
  *inv_T = 1.0f / p->temperature;
  if (!(*inv_T > 0.0f) || !std::isfinite(*inv_T)) return fail(TTX_ERR_INVALID, w + ": 1 / temperature is not a positive finite fp32");
  *top_k = 0; *top_p = 1.0f;
  if (!f) return TTX_OK;
  if (f->top_k < 0 || f->top_k > SAMPLE_MAX_KEEP) return fail(TTX_ERR_INVALID, x + ": top_k must be 0 or in [1, 32]");
  if (!(f->top_p > 0.0f) || !(f->top_p <= 1.0f)) return fail(TTX_ERR_INVALID, x + ": top_p must be in (0, 1]");
  *top_p = f->top_p;
  *top_k = (f->top_k == 0 && f->top_p < 1.0f) ? SAMPLE_MAX_KEEP : f->top_k;
  return TTX_OK;
}

// Stochastic beam search: the standard beam loop above with k_sbs_step (csrc/ttx_sbs.hip.h) where it launches k_beam_step; with a
// filter on or a non-empty prefix k_sbs_step_masked.  A call with no filter, no prefix and no bias is the plain one, launch for launch.
static int sbs_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sbs_params* p,
                        const ttx_sbs_filter* f, const ttx_sample_opts& o, int64_t* d_out, float* d_logp, float* d_gumbel,
                        const ttx_sbs_trace* trace, ttx_beam_search_stats* stats, void* stream) {
  const Who who("ttx_sbs_generate", "ttx_sbs_generate_ex", "ttx_sbs_generate_bias", "ttx_sbs_generate");
  if (!s || !d_src || !p || !d_out || !d_logp || !d_gumbel || !stats || B <= 0 || Ls <= 1)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_sbs_generate");
  float inv_T, top_p;
  int top_k;
  TTX_TRY(sbs_validate(who, s->m->cfg, p, f, &inv_T, &top_k, &top_p));
  if (trace && (!trace->d_parent || !trace->d_token || !trace->d_phi || !trace->d_g))
    return fail(TTX_ERR_INVALID, "ttx_sbs_generate: a trace needs all four arrays");
  SampleSetup c{};
  TTX_TRY(constraints_validate(who, s, o, nullptr, B, p->max_len, &c));
  ttx_beam_search_params bp{};
  bp.max_len = p->max_len; bp.beam_size = p->beam_size; bp.pad_token = p->pad_token; bp.bos_token = p->bos_token; bp.eos_token = p->eos_token;
  BeamSearchJob j;
  return bsearch_drive(j, s, stats, stream, [&](int) -> int {
    TTX_TRY(bsearch_constraints_ensure(s, s->own_stream, c, B, p->max_len));
    TTX_TRY(bsearch_start(j, s, s->own_stream, d_src, B, Ls, &bp, d_out, true));
    j.inv_T = inv_T; j.seed = p->seed; j.row_keys = d_row_keys; j.d_logp = d_logp; j.d_gumbel = d_gumbel;
    if (trace) j.trace = *trace;
    j.masked = top_k > 0 || c.prompted; j.top_k = top_k; j.top_p = top_p;
    TTX_TRY(bsearch_constraints_upload(j, c));
    return bsearch_launch_iter(j);
  });
}

extern "C" int ttx_sbs_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sbs_params* p,
                                int64_t* d_out, float* d_logp, float* d_gumbel, const ttx_sbs_trace* trace, ttx_beam_search_stats* stats,
                                void* stream) {
  return sbs_generate(s, d_src, B, Ls, d_row_keys, p, nullptr, NO_OPTS, d_out, d_logp, d_gumbel, trace, stats, stream);
}

extern "C" int ttx_sbs_generate_ex(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sbs_params* p,
                                   const ttx_sbs_filter* f_or_null, const int64_t* d_prefix, int ld_prefix, const int32_t* h_prefix_len,
                                   int64_t* d_out, float* d_logp, float* d_gumbel, const ttx_sbs_trace* trace,
                                   ttx_beam_search_stats* stats, void* stream) {
  return sbs_generate(s, d_src, B, Ls, d_row_keys, p, f_or_null, opts_of(d_prefix, ld_prefix, h_prefix_len, nullptr, 0, nullptr), d_out, d_logp,
                      d_gumbel, trace, stats, stream);
}

// The general form: ttx_sbs_generate_ex under a per-source logit bias, k_logit_bias on every level's logits before the step kernel
// reads them.
extern "C" int ttx_sbs_generate_bias(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sbs_params* p,
                                     const ttx_sbs_filter* f_or_null, const int64_t* d_prefix, int ld_prefix, const int32_t* h_prefix_len,
                                     const float* d_bias, int ld_bias, int64_t* d_out, float* d_logp, float* d_gumbel,
                                     const ttx_sbs_trace* trace, ttx_beam_search_stats* stats, void* stream) {
  ttx_sample_opts o = opts_of(d_prefix, ld_prefix, h_prefix_len, nullptr, 0, nullptr);
  o.d_bias = d_bias; o.ld_bias = ld_bias;
  return sbs_generate(s, d_src, B, Ls, d_row_keys, p, f_or_null, o, d_out, d_logp, d_gumbel, trace, stats, stream);
}

// ------------------------------------------------------------------------------------------------
// Stochastic beam search on a pool of source slots (kernels, slot state and the argument for exactness: csrc/ttx_sbs_pool.hip.h).
// Host side: one job per session, each a pool of C source slots fed from the caller's list of sources; an iteration is one fixed
// linear launch sequence (captured once per cache parity and GEMM variant) over every unfinished candidate in the pool.
struct SbsPoolJob {
  ttx_session* s = nullptr;
  hipStream_t st = nullptr;
  ttx_sbs_params p{};
  int C = 0, K = 0, MC = 0, ld = 0, Lc = 0, Ls_cap = 0;
  float inv_T = 1.f;
  bool masked = false, prompted = false;
  int top_k = 0; float top_p = 1.f;
  SbsPoolArgs a{};                  // g_in / g_out unset: sbsp_args(j, parity) fills them
  SbsPoolStepArgs sa{};             // g / new_g likewise
  PoolState pool;                   // launched: iterations enqueued (pool_step, ttx_admit.h)
  int cur = 0;                      // the parity of the iteration to come (cache buffer read, G buffer read)
  long long src_tokens_padded = 0, live_slots = 0;
  SbsPoolIo io{};                   // host image of the session's device block
};

static SbsPoolArgs sbsp_args(const SbsPoolJob& j, int parity) {
  float* const gbuf[2] = {j.s->sbs_g.as<float>(), j.s->sbs_g_next.as<float>()};
  SbsPoolArgs a = j.a;
  a.g_in = gbuf[parity]; a.g_out = gbuf[parity ^ 1];
  return a;
}

static int launch_sbsp_init(hipStream_t st, const SbsPoolArgs& a, float* g_a, float* g_b, int* src_of) {
  hipLaunchKernelGGL(k_sbsp_init, dim3(64), dim3(256), 0, st, a, g_a, g_b, src_of);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_sbsp_admit(hipStream_t st, const SbsPoolArgs& a, int* new_slot, int R, int first_row) {
  hipLaunchKernelGGL(k_sbsp_admit, dim3(1), dim3(1), 0, st, a, new_slot, R, first_row);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_sbsp_fill(hipStream_t st, const SbsPoolFillArgs& f) {
  hipLaunchKernelGGL(k_sbsp_fill, dim3(f.R, 1 + f.Ls_new), dim3(256), 0, st, f);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_sbsp_retire(hipStream_t st, const SbsPoolArgs& a) {
  hipLaunchKernelGGL(k_sbsp_retire, dim3(a.C), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_sbsp_publish(hipStream_t st, const SbsPoolArgs& a) {
  hipLaunchKernelGGL(k_sbsp_publish, dim3(1), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

static int launch_sbs_step_pool(ttx_session* s, hipStream_t st, const SbsPoolStepArgs& sa) {
  const size_t lds = (size_t)sa.K * sa.V * 4;
  TTX_TRY(raise_lds_limit(reinterpret_cast<const void*>(&k_sbs_step_pool), lds, s->attr_sbs_step_pool));
  hipLaunchKernelGGL(k_sbs_step_pool, dim3(sa.C), dim3(256), lds, st, sa);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

template <int VPL>
static int launch_sbs_step_pool_masked_vpl(hipStream_t st, const SbsPoolStepArgs& sa, int waves, bool& attr) {
  const size_t lds = (size_t)sa.K * sa.V * 4;
  TTX_TRY(raise_lds_limit(reinterpret_cast<const void*>(&k_sbs_step_pool_masked<VPL>), lds, attr));
  hipLaunchKernelGGL((k_sbs_step_pool_masked<VPL>), dim3(sa.C), dim3(64 * waves), lds, st, sa);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// The wave count follows K (a slot's parent count is 1 or K; no sum or maximum changes its order with the wave count).
static int launch_sbs_step_pool_masked(ttx_session* s, hipStream_t st, const SbsPoolStepArgs& sa) {
  const int waves = sbs_masked_waves(sa.K);
  if (sa.V <= 64) return launch_sbs_step_pool_masked_vpl<1>(st, sa, waves, s->attr_sbs_step_pool_masked[0]);
  if (sa.V <= 128) return launch_sbs_step_pool_masked_vpl<2>(st, sa, waves, s->attr_sbs_step_pool_masked[1]);
  if (sa.V <= 256) return launch_sbs_step_pool_masked_vpl<4>(st, sa, waves, s->attr_sbs_step_pool_masked[2]);
  if (sa.V <= 512) return launch_sbs_step_pool_masked_vpl<8>(st, sa, waves, s->attr_sbs_step_pool_masked[3]);
  return launch_sbs_step_pool_masked_vpl<16>(st, sa, waves, s->attr_sbs_step_pool_masked[4]);
}

// What every pool of a call is started with; `c`: the call's constraints, of which the pool takes the prefix alone
struct SbsPoolCall {
  const int32_t* h_len; const int64_t* d_row_keys; int S_total;
  SampleSetup c;
  int64_t* d_out; float* d_logp; float* d_gumbel; int32_t* d_src_running;
};

static int sbsp_start(SbsPoolJob& j, ttx_session* s, hipStream_t st, int C, int Ls_cap, const ttx_sbs_params* p, float inv_T, int top_k,
                      float top_p, const SbsPoolCall& call) {
  const ttx_config& c = s->m->cfg;
  const int d = c.embedding_dim, Ld = c.num_decoder_layers, K = p->beam_size, S = call.S_total;
  j = SbsPoolJob{};
  j.s = s; j.st = st; j.p = *p; j.C = C; j.K = K; j.MC = C * K; j.ld = p->max_len + 2; j.Lc = p->max_len + 2; j.Ls_cap = Ls_cap;
  j.inv_T = inv_T; j.top_k = top_k; j.top_p = top_p; j.prompted = call.c.prompted; j.masked = top_k > 0 || call.c.prompted;
  const size_t MC = (size_t)j.MC;
  Needs need{st};
  need_source_slots(s, need, C, Ls_cap);
  need(s->bp_enc_qkv, (size_t)C * Ls_cap * 3 * d * 4);      // admissions must not touch the step's Q/K/V rows (k_tree_cache reads them)
  need(s->drafts, MC * 4);
  need(s->gen, MC * j.ld * 4); need(s->front, MC * 4); need(s->act_idx, MC * 4);
  for (int i = 0; i < 2; ++i) { need(s->tk[i], (size_t)Ld * MC * j.Lc * d * 4); need(s->tv[i], (size_t)Ld * MC * j.Lc * d * 4); }
  need(s->t_prev_len, MC * 4); need(s->t_slot_of, MC * 4); need(s->t_src_of, MC * 4); need(s->bp_cand_len, MC * 4);
  need(s->bs_cand_next, MC * j.ld * 8); need(s->bs_len_next, MC * 4); need(s->bs_fin_next, MC); need(s->bs_logp_next, MC * 4);
  need(s->bs_len, MC * 4); need(s->bs_fin, MC); need(s->bs_active, MC); need(s->bs_logp, MC * 4); need(s->bs_per_cand, MC * 4);
  need(s->bs_parent, MC * 4); need(s->bs_parent_draft, MC * 4); need(s->bs_cnt, sizeof(BeamCounters)); need(s->beam_summary, 8 * 4);
  need(s->sbs_g, MC * 4); need(s->sbs_g_next, MC * 4);
  need(s->sbp_slot, (size_t)C * (8 + 7 * 4)); need(s->sbp_len, (size_t)S * 4); need(s->bp_new_slot, (size_t)C * 4); need(s->bp_grp, 4 * 4);
  need(s->sbp_io, sizeof(SbsPoolIo));
  if (need.rc == TTX_OK) need.rc = constraints_ensure(s, st, call.c, p->max_len, 0, 0, 0);
  need_step_workspaces(s, need, MC, (size_t)C * Ls_cap);
  s->graphs_current();
  TTX_TRY(need.rc);
  BeamPoolHost* dev_host = nullptr;
  TTX_TRY(pool_host_begin(s, st, &dev_host));
  HIP_TRY(hipMemcpyAsync(s->sbp_len.p, call.h_len, (size_t)S * 4, hipMemcpyHostToDevice, st));
  SbsPoolArgs& a = j.a;
  a.C = C; a.K = K; a.max_len = p->max_len; a.ld = j.ld; a.Ls_cap = Ls_cap; a.pad = p->pad_token; a.bos = p->bos_token;
  a.key = s->sbp_slot.as<int64_t>();
  a.row_of = reinterpret_cast<int*>(a.key + C); a.level = a.row_of + C; a.nlive = a.row_of + 2 * C; a.nfin = a.row_of + 3 * C;
  a.pfx_len = a.row_of + 4 * C; a.pfx_src = a.row_of + 5 * C; a.run_acc = a.row_of + 6 * C;
  ConstraintTabs t;                         // a slot's prefix length and its row of the table are written at admission
  TTX_TRY(constraints_upload(s, st, call.c, p->max_len, p->pad_token, a.pfx_len, a.pfx_src, nullptr, &t));
  a.cand_next = s->bs_cand_next.as<int64_t>(); a.len_next = s->bs_len_next.as<int>(); a.fin_next = s->bs_fin_next.as<uint8_t>();
  a.phi_next = s->bs_logp_next.as<float>(); a.parent = s->bs_parent.as<int>(); a.parent_draft = s->bs_parent_draft.as<int>();
  a.cand_src_len = s->bp_cand_len.as<int>();
  a.len_all = s->sbp_len.as<int>(); a.row_keys = call.d_row_keys; a.pfx_len_src = j.prompted ? s->pfx_len_src.as<int>() : nullptr;
  j.io = SbsPoolIo{call.d_out, call.d_logp, call.d_gumbel, call.d_src_running};
  HIP_TRY(hipMemcpyAsync(s->sbp_io.p, &j.io, sizeof(SbsPoolIo), hipMemcpyHostToDevice, st));
  a.io = s->sbp_io.as<SbsPoolIo>();
  a.cnt = s->bs_cnt.as<BeamCounters>(); a.host = dev_host; a.dev_summary = s->bp_grp.as<int>();
  SbsPoolStepArgs& sa = j.sa;
  sa.logits = s->logits.as<float>(); sa.V = c.vocab_size; sa.slot_of = s->t_slot_of.as<int>(); sa.finished = s->bs_fin.as<uint8_t>();
  sa.phi = s->bs_logp.as<float>(); sa.gen = s->gen.as<int>(); sa.ld = j.ld; sa.C = C; sa.K = K; sa.pad = p->pad_token; sa.eos = p->eos_token;
  sa.row_of = a.row_of; sa.level = a.level; sa.nlive = a.nlive; sa.key = a.key; sa.seed = p->seed; sa.inv_T = inv_T;
  sa.new_cand = a.cand_next; sa.new_phi = a.phi_next; sa.parent = a.parent; sa.new_len = a.len_next; sa.new_finished = a.fin_next;
  sa.parent_draft = a.parent_draft; sa.nfin = a.nfin;
  sa.top_k = top_k; sa.top_p = top_p;
  sa.pfx = t.pfx;
  TTX_TRY(launch_sbsp_init(st, a, s->sbs_g.as<float>(), s->sbs_g_next.as<float>(), s->t_src_of.as<int>()));
  HIP_TRY(hipEventRecord(s->ev_b, st));
  j.pool.phase = 1;
  return TTX_OK;
}

// Encode R new sources (rows first_row .. of the caller's matrix, Ls_new columns of it) and hand them free slots.
static int sbsp_admit(SbsPoolJob& j, const int64_t* d_src_rows, int ld_src, int R, int Ls_new, int first_row) {
  ttx_session* s = j.s;
  hipStream_t st = j.st;
  TTX_TRY(encode_sources(s, st, d_src_rows, ld_src, R, Ls_new, s->valid_new.as<uint8_t>(), s->memkv_new.as<float>(), s->bp_enc_qkv.as<float>()));
  SbsPoolFillArgs f{};
  f.a = sbsp_args(j, j.cur);                  // G = 0 goes where the next iteration reads it
  f.new_slot = s->bp_new_slot.as<int>(); f.R = R; f.first_row = first_row; f.Ls_new = Ls_new;
  f.src_valid = s->src_valid.as<uint8_t>(); f.valid_new = s->valid_new.as<uint8_t>();
  f.memkv = s->memkv.as<float>(); f.memkv_new = s->memkv_new.as<float>(); f.kv_row = s->m->cfg.num_decoder_layers * 2 * s->m->cfg.embedding_dim;
  TTX_TRY(launch_sbsp_admit(st, f.a, s->bp_new_slot.as<int>(), R, first_row));
  TTX_TRY(launch_sbsp_fill(st, f));
  j.src_tokens_padded += (long long)R * Ls_new;
  return TTX_OK;
}

static int sbsp_enqueue_iter(const SbsPoolJob& j, int variant) {
  ttx_session* s = j.s;
  hipStream_t st = j.st;
  const int cur = j.cur, max_len = j.p.max_len;
  BeamPrepArgs pa{};
  pa.ld = j.ld; pa.n_cand = j.MC; pa.beam = j.K; pa.dl = 0; pa.N = 1; pa.pad = j.p.pad_token; pa.smart = 0;
  TTX_TRY(enqueue_bs_prep(s, st, j.MC, pa));
  TTX_TRY(enqueue_tree_cache(s, st, j.MC, j.Lc, cur, cur ^ 1, nullptr, nullptr, 1, 0));      // fresh candidates (parent -1) inherit nothing
  TTX_TRY(enqueue_bs_list(s, st, j.MC, 1, 0));
  StepCtx k = tree_step_ctx(s, j.MC, j.Ls_cap, 1, 0, j.Lc, j.ld, max_len, cur ^ 1, variant);
  k.src_len = s->bp_cand_len.as<int>();
  TTX_TRY(run_step(s, st, k, key_capacity(max_len, max_len)));
  const SbsPoolArgs a = sbsp_args(j, cur);
  SbsPoolStepArgs sa = j.sa;
  sa.g = a.g_in; sa.new_g = const_cast<float*>(a.g_out);
  if (j.masked) TTX_TRY(launch_sbs_step_pool_masked(s, st, sa));
  else TTX_TRY(launch_sbs_step_pool(s, st, sa));
  TTX_TRY(launch_sbsp_retire(st, a));
  return launch_sbsp_publish(st, a);
}

static int sbsp_launch_iter(SbsPoolJob& j, int n_running) {
  ttx_session* s = j.s;
  const int variant = variant_for_rows(s, (long long)std::max(1, n_running), true);
  int inv_T_bits = 0, top_p_bits = 0;
  std::memcpy(&inv_T_bits, &j.inv_T, 4); std::memcpy(&top_p_bits, &j.top_p, 4);
  const GraphKey key{GS_SBS_POOL_ITER, j.C, j.Ls_cap, j.K, j.p.max_len, j.cur, variant, j.p.pad_token, j.p.bos_token, j.p.eos_token,
                     j.masked ? 1 : 0, j.prompted ? 1 : 0, j.top_k, top_p_bits, inv_T_bits, (int)(unsigned)j.p.seed, (int)(unsigned)(j.p.seed >> 32)};
  TTX_TRY(graph_replay(s, j.st, s->iter_graphs, key, [&]() -> int { return sbsp_enqueue_iter(j, variant); }));
  ++j.pool.launched;
  j.cur ^= 1;
  return TTX_OK;
}

extern "C" int ttx_sbs_generate_pool(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total, int Ls_all,
                                     const int32_t* h_len, const int64_t* d_row_keys, int capacity, const ttx_sbs_params* p,
                                     const ttx_sbs_filter* f, const int64_t* d_prefix, int ld_prefix, const int32_t* h_prefix_len,
                                     int64_t* d_out, float* d_logp, float* d_gumbel, ttx_sbs_pool_stats* stats, void* stream) {
  const std::string who = "ttx_sbs_generate_pool";
  if (!sessions || n_sessions <= 0 || !d_src || S_total < 0 || Ls_all <= 1 || !h_len || !p || !d_out || !d_logp || !d_gumbel || !stats)
    return fail(TTX_ERR_INVALID, "bad argument to " + who);
  for (int i = 0; i < n_sessions; ++i) if (!sessions[i]) return fail(TTX_ERR_INVALID, who + ": null session");
  if (capacity < 1 || capacity > 1024) return fail(TTX_ERR_INVALID, who + ": capacity must lie in [1, 1024]");
  const ttx_config& c = sessions[0]->m->cfg;
  float inv_T, top_p;
  int top_k;
  TTX_TRY(sbs_validate(who.c_str(), c, p, f, &inv_T, &top_k, &top_p));
  if ((size_t)p->beam_size * c.vocab_size * 4 > 150 * 1024)
    return fail(TTX_ERR_INVALID, who + ": beam_size x vocabulary beyond the selection kernel's LDS image");
  if (p->pad_token != c.pad_token) return fail(TTX_ERR_INVALID, who + ": generator pad token differs from the model's");
  if (p->max_len + 2 > c.max_positions) return fail(TTX_ERR_INVALID, who + ": max_len exceeds the positional table");
  int len_max = 2;
  for (int i = 0; i < S_total; ++i) {
    if (h_len[i] < 2 || h_len[i] > Ls_all) return fail(TTX_ERR_INVALID, who + ": source length outside [2, width of the source matrix]");
    len_max = std::max(len_max, (int)h_len[i]);
  }
  const int Ls_cap = pool_slot_width(len_max, c.max_positions);
  if (Ls_cap > c.max_positions) return fail(TTX_ERR_INVALID, who + ": source longer than the positional table");
  SbsPoolCall call{};
  call.h_len = h_len; call.d_row_keys = d_row_keys; call.S_total = S_total; call.d_out = d_out; call.d_logp = d_logp; call.d_gumbel = d_gumbel;
  TTX_TRY(constraints_validate(who.c_str(), sessions[0], opts_of(d_prefix, ld_prefix, h_prefix_len, nullptr, 0, nullptr), nullptr, S_total,
                               p->max_len, &call.c));
  call.d_src_running = stats->d_src_running_rows;           // the one input of the block
  *stats = ttx_sbs_pool_stats{};
  stats->d_src_running_rows = call.d_src_running;
  if (S_total == 0) return TTX_OK;
  const PoolShape shape = pool_shape(n_sessions, S_total, S_total, capacity, 8, 1);      // the work list: sources
  const int n_jobs = shape.n_jobs, C = shape.C;
  std::vector<int> first(S_total + 1);
  for (int r = 0; r <= S_total; ++r) first[r] = r;
  PoolList list = pool_list(first.data(), S_total, n_jobs);
  std::vector<SbsPoolJob> jobs(n_jobs);
  const bool serial = sessions[0]->profile;                    // profiling sessions: one pool after another (see the greedy pool)
  const long long max_launches = (long long)p->max_len * (S_total + 1);
  ttx_sbs_pool_stats acc{};
  acc.d_src_running_rows = call.d_src_running;
  const auto start = [&](int i) -> int {
    return sbsp_start(jobs[i], sessions[i], sessions[i]->own_stream, C, Ls_cap, p, inv_T, top_k, top_p, call);
  };
  const auto turn = [&](int i) -> int {
    SbsPoolJob& j = jobs[i];
    ttx_session* s = j.s;
    if (j.pool.phase == 1) {
      const PoolPlan plan = pool_step(j.pool, list, pool_look(s->bp_host, j.pool.launched), i, C, serial, max_launches);
      switch (plan.act) {
        case PoolPlan::WAIT: return TURN_WAITING;
        case PoolPlan::FAILED: return fail(TTX_ERR_HIP, "stochastic beam pool bookkeeping failed (admitted more sources than free slots)");
        case PoolPlan::STUCK: return fail(TTX_ERR_HIP, "stochastic beam pool failed to terminate");
        case PoolPlan::DRAIN:
          TTX_TRY(enqueue_readback(s, j.st, s->bs_cnt.p, sizeof(BeamCounters)));
          j.pool.phase = 2;
          break;
        case PoolPlan::LAUNCH:
          if (plan.n_take > 0)
            TTX_TRY(sbsp_admit(j, d_src + (size_t)plan.first_row * Ls_all, Ls_all, plan.rows,
                               chunk_width(h_len, plan.first_row, plan.first_row + plan.rows), plan.first_row));
          j.live_slots += plan.n_live;
          TTX_TRY(sbsp_launch_iter(j, plan.n_running));
          break;
      }
      return TURN_PROGRESSED;
    }
    if (hipEventQuery(s->ev_done) != hipSuccess) return TURN_IDLE;
    const BeamCounters* cn = reinterpret_cast<const BeamCounters*>(s->host_state);
    acc.model_calls += cn->model_calls; acc.running_rows += cn->running_cands; acc.src_tokens_padded += j.src_tokens_padded;
    acc.live_slots += j.live_slots;
    pool_finish(s, j.st, &acc.decode_ms);
    j.pool.phase = 3;
    return TURN_FINISHED;
  };
  acc.status = drive_sessions(sessions, n_jobs, serial, stream, start, turn);
  *stats = acc;
  return acc.status;
}

// Parity instrumentation: the verify step selected by ttx_gen_params.want_logits (1-based step number) of the most
// recent generate call on this session: its pre-argmax logits and the loop state they were computed from.
// All destinations are HOST pointers; sizes: logits [n_active*rps, V], act [n_active], front [B], gen [B, gen_ld].
// info[0..5] = n_active, rps (rows per sequence = 1 + N*D), B, gen_ld, V, step.  Pass nulls to query info only.
extern "C" int ttx_debug_step_snapshot(ttx_session* s, int32_t* info, float* h_logits, int32_t* h_act, int32_t* h_front,
                                       int32_t* h_gen) {
  if (!s || !info) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_step_snapshot");
  if (s->snap_step == 0) return fail(TTX_ERR_INVALID, "no verify step was recorded (set ttx_gen_params.want_logits)");
  HIP_TRY(hipSetDevice(s->m->device));
  HIP_TRY(hipDeviceSynchronize());
  DecState st;
  HIP_TRY(hipMemcpy(&st, s->snap_state.p, sizeof(DecState), hipMemcpyDeviceToHost));
  const int V = s->m->cfg.vocab_size;
  info[0] = st.n_active; info[1] = s->snap_rps; info[2] = s->snap_B; info[3] = s->snap_gen_ld; info[4] = V; info[5] = s->snap_step;
  if (h_logits) HIP_TRY(hipMemcpy(h_logits, s->snap_logits.p, (size_t)st.n_active * s->snap_rps * V * 4, hipMemcpyDeviceToHost));
  if (h_act) HIP_TRY(hipMemcpy(h_act, s->snap_act.p, (size_t)st.n_active * 4, hipMemcpyDeviceToHost));
  if (h_front) HIP_TRY(hipMemcpy(h_front, s->snap_front.p, (size_t)s->snap_B * 4, hipMemcpyDeviceToHost));
  if (h_gen) HIP_TRY(hipMemcpy(h_gen, s->snap_gen.p, (size_t)s->snap_B * s->snap_gen_ld * 4, hipMemcpyDeviceToHost));
  return TTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Host-side tokenizer / collate / detokenizer (no GPU)
extern "C" int ttx_tokenizer_create(const char* const* tokens, const int32_t* ids, int n, ttx_tokenizer** out) {
  if (!tokens || !ids || n <= 0 || !out) return fail(TTX_ERR_INVALID, "bad argument to ttx_tokenizer_create");
  ttx_tokenizer* t = new ttx_tokenizer();
  int32_t max_id = -1;
  for (int i = 0; i < n; ++i) max_id = std::max(max_id, ids[i]);
  t->dec.assign((size_t)max_id + 1, std::string());
  for (int i = 0; i < n; ++i) {
    if (!tokens[i] || ids[i] < 0) { delete t; return fail(TTX_ERR_INVALID, "vocabulary entry with a null token or negative id"); }
    t->enc[tokens[i]] = ids[i];
    t->dec[ids[i]] = tokens[i];
  }
  *out = t;
  return TTX_OK;
}

extern "C" void ttx_tokenizer_destroy(ttx_tokenizer* t) { delete t; }

// ChemSMILESTokenizer.encode: returns the number of ids the line needs (BOS and EOS included); writes min(that, cap).
extern "C" int ttx_tokenizer_encode(const ttx_tokenizer* t, const char* line, int32_t* out, int cap) {
  if (!t || !line) return fail(TTX_ERR_INVALID, "null argument to ttx_tokenizer_encode");
  int n = 0;
  auto put = [&](int32_t id) { if (out && n < cap) out[n] = id; ++n; };
  put(t->bos);
  std::string piece;
  ttxtok::split(line, std::strlen(line), [&](const char* p, size_t len) {
    piece.assign(p, len);
    auto it = t->enc.find(piece);
    put(it == t->enc.end() ? t->unk : it->second);
  });
  put(t->eos);
  return n;
}

// Tokenize B lines and pad them to the longest (the DataModule's collate: seq2seq_wrappers.py:121-127).  `out` is int64
// [B, cap_cols] row-major (HOST); returns the padded width (<= cap_cols) or, if some line needs more columns, minus the
// width required (nothing usable is written then).
extern "C" int ttx_tokenizer_encode_batch(const ttx_tokenizer* t, const char* const* lines, int B, int64_t* out, int cap_cols) {
  if (!t || !lines || B <= 0 || !out || cap_cols <= 0) return fail(TTX_ERR_INVALID, "bad argument to ttx_tokenizer_encode_batch");
  std::vector<int32_t> row((size_t)cap_cols);
  int width = 0;
  for (int b = 0; b < B; ++b) {
    const int n = ttx_tokenizer_encode(t, lines[b], row.data(), cap_cols);
    if (n < 0) return n;
    width = std::max(width, n);
    if (n <= cap_cols) {
      for (int i = 0; i < n; ++i) out[(size_t)b * cap_cols + i] = row[i];
      for (int i = n; i < cap_cols; ++i) out[(size_t)b * cap_cols + i] = t->pad;
    }
  }
  return width <= cap_cols ? width : -width;
}

// GenericTokenizer.decode with skip_service_tokens=True: returns the string length (NUL excluded) the ids need; writes at
// most cap-1 characters and a terminating NUL.  Ids outside the vocabulary fail (the reference raises KeyError).
extern "C" int ttx_tokenizer_decode(const ttx_tokenizer* t, const int64_t* ids, int n, char* out, int cap) {
  if (!t || (!ids && n > 0)) return fail(TTX_ERR_INVALID, "null argument to ttx_tokenizer_decode");
  size_t len = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t id = ids[i];
    if (id != t->bos && id != t->eos && id != t->pad) {
      if (id < 0 || (size_t)id >= t->dec.size() || (t->dec[id].empty() && t->enc.find("") == t->enc.end()))
        return fail(TTX_ERR_REFERENCE, "token id outside the vocabulary (KeyError in the reference)");
      const std::string& tok = t->dec[id];
      for (char ch : tok) { if (out && (int)len + 1 < cap) out[len] = ch; ++len; }
    }
    if (id == t->eos) break;
  }
  if (out && cap > 0) out[std::min(len, (size_t)cap - 1)] = '\0';
  return (int)len;
}

// Development aid (tools/bench_gemm.py): one GEMM shape in isolation (ttx_gemm.hip: gemm_bench).
extern "C" int ttx_debug_gemm_bench(ttx_session* s, int M, int N, int K, int splits, int variant, int reps, double* us_per_launch,
                                    double* max_abs_diff) {
  return gemm_bench(s, M, N, K, splits, variant, reps, us_per_launch, max_abs_diff);
}

// Test entry points: one GEMM / finisher launch on the caller's device operands (ttx_gemm.hip: gemm_debug, finish_debug).
extern "C" int ttx_debug_gemm_act(ttx_session* s, const float* d_x, int ldx, const float* d_w, int ldw, const float* d_bias, float* d_y,
                                  int ldy, const int32_t* d_m, int m_max, int N, int K, int activation, int splits, int64_t slab_stride,
                                  int variant, int tiling, int32_t* kernel_id, void* stream) {
  return gemm_debug(s, d_x, ldx, d_w, ldw, d_bias, d_y, ldy, d_m, m_max, N, K, activation, splits, (long long)slab_stride, variant,
                    tiling, kernel_id, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int ttx_debug_gemm(ttx_session* s, const float* d_x, int ldx, const float* d_w, int ldw, const float* d_bias, float* d_y,
                              int ldy, const int32_t* d_m, int m_max, int N, int K, int relu, int splits, int64_t slab_stride,
                              int variant, int tiling, int32_t* kernel_id, void* stream) {
  return ttx_debug_gemm_act(s, d_x, ldx, d_w, ldw, d_bias, d_y, ldy, d_m, m_max, N, K, relu ? TTX_ACT_RELU : TTX_ACT_NONE, splits,
                            slab_stride, variant, tiling, kernel_id, stream);
}

extern "C" int ttx_debug_finish_ln(ttx_session* s, const float* d_slabs, int n_slabs, int64_t slab_stride, const float* d_bias,
                                   const float* d_resid, const float* d_g1, const float* d_b1, const float* d_g2, const float* d_b2,
                                   const uint8_t* d_row_valid, float* d_y, const int32_t* d_m, int m_max, int d, float eps,
                                   void* stream) {
  return finish_debug(s, d_slabs, n_slabs, (long long)slab_stride, d_bias, d_resid, d_g1, d_b1, d_g2, d_b2, d_row_valid, d_y, d_m,
                      m_max, d, eps, reinterpret_cast<hipStream_t>(stream));
}

// Test entry point: one attention launch on the caller's device operands (ttx_attn.hip: attn_debug).
extern "C" int ttx_debug_attn_hd(ttx_session* s, const float* d_q, int ldq, const float* d_k, const float* d_v, int ldkv, float* d_out,
                                 int H, int head_dim, float scale, int L, int Lk, const int32_t* d_tok, int pad, const uint8_t* d_key_pad,
                                 const int32_t* d_mem_row, const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_src_of,
                                 const int32_t* d_src_len, const float* d_kcache, const float* d_vcache, int64_t cache_seq_stride,
                                 const int32_t* d_cache_slot, int gen_ld, int N, int D, int mode, int groups, int n_active, int max_keys,
                                 int kernel, int32_t* kernel_id, void* stream) {
  AttnArgs a{};
  a.q = d_q; a.ldq = ldq; a.k = d_k; a.v = d_v; a.ldkv = ldkv; a.out = d_out; a.scale = scale; a.L = L; a.Lk = Lk;
  a.tok = d_tok; a.pad = pad; a.key_pad = d_key_pad; a.mem_row = d_mem_row; a.act_idx = d_act_idx; a.front = d_front;
  a.src_of = d_src_of; a.src_len = d_src_len; a.kcache = d_kcache; a.vcache = d_vcache; a.cache_seq_stride = (long long)cache_seq_stride;
  a.cache_slot = d_cache_slot; a.gen_ld = gen_ld; a.N = N; a.D = D;
  return attn_debug(s, a, H, head_dim, mode, groups, n_active, max_keys, kernel, kernel_id, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int ttx_debug_attn_as(ttx_session* s, const float* d_q, int ldq, const float* d_k, const float* d_v, int ldkv, float* d_out,
                                 int H, int head_dim, float scale, int L, int Lk, const int32_t* d_tok, int pad, const uint8_t* d_key_pad,
                                 const int32_t* d_mem_row, const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_src_of,
                                 const int32_t* d_src_len, const float* d_kcache, const float* d_vcache, int64_t cache_seq_stride,
                                 const int32_t* d_cache_slot, int gen_ld, int N, int D, int mode, int groups, int n_active, int max_keys,
                                 int kernel, int32_t* kernel_id, int sel_N, int sel_D, void* stream) {
  if (!s) return fail(TTX_ERR_INVALID, "null session");
  if (sel_N < 1 || sel_D < 0) return fail(TTX_ERR_INVALID, "ttx_debug_attn_as: the layout to choose as needs N >= 1 and D >= 0");
  s->attn_sel_N = sel_N; s->attn_sel_D = sel_D;
  const int rc = ttx_debug_attn_hd(s, d_q, ldq, d_k, d_v, ldkv, d_out, H, head_dim, scale, L, Lk, d_tok, pad, d_key_pad, d_mem_row, d_act_idx,
                                   d_front, d_src_of, d_src_len, d_kcache, d_vcache, cache_seq_stride, d_cache_slot, gen_ld, N, D, mode,
                                   groups, n_active, max_keys, kernel, kernel_id, stream);
  s->attn_sel_N = 0; s->attn_sel_D = 0;
  return rc;
}

extern "C" int ttx_debug_attn(ttx_session* s, const float* d_q, int ldq, const float* d_k, const float* d_v, int ldkv, float* d_out,
                              int H, float scale, int L, int Lk, const int32_t* d_tok, int pad, const uint8_t* d_key_pad,
                              const int32_t* d_mem_row, const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_src_of,
                              const int32_t* d_src_len, const float* d_kcache, const float* d_vcache, int64_t cache_seq_stride,
                              const int32_t* d_cache_slot, int gen_ld, int N, int D, int mode, int groups, int n_active, int max_keys,
                              int kernel, int32_t* kernel_id, void* stream) {
  return ttx_debug_attn_hd(s, d_q, ldq, d_k, d_v, ldkv, d_out, H, 32, scale, L, Lk, d_tok, pad, d_key_pad, d_mem_row, d_act_idx, d_front,
                           d_src_of, d_src_len, d_kcache, d_vcache, cache_seq_stride, d_cache_slot, gen_ld, N, D, mode, groups, n_active,
                           max_keys, kernel, kernel_id, stream);
}

// Draft select (tests/test_gpu_draft_select.py): the per-position operands of a compacted draft pass, read back and checked as the
// other index arrays of the test entry points are.  mask[p] is a non-zero subset of the N drafts and row_base the exclusive prefix
// sum of 1 + D * popcount(mask); hands back the compacted row count.
static int dbg_check_select(const std::string& who, const int32_t* d_row_base, const int32_t* d_draft_mask, int n, int N, int D,
                            hipStream_t st, std::vector<int32_t>* mask_out, int* total) {
  *total = 0;
  if (!d_row_base || !d_draft_mask) return fail(TTX_ERR_INVALID, who + ": row_base and draft_mask are required");
  if (N < 1 || N > 32 || D < 1) return fail(TTX_ERR_INVALID, who + ": draft select needs 1 <= N <= 32 and D >= 1");
  std::vector<int32_t> base((size_t)std::max(n, 1)), mask((size_t)std::max(n, 1));
  if (n > 0) {
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(base.data(), d_row_base, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mask.data(), d_draft_mask, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  int sum = 0;
  for (int p = 0; p < n; ++p) {
    const unsigned m = (unsigned)mask[p];
    if (m == 0u || (N < 32 && (m >> N))) return fail(TTX_ERR_INVALID, who + ": a listed slot's draft mask must be a non-zero subset of the N drafts");
    if (base[p] != sum) return fail(TTX_ERR_INVALID, who + ": row_base must be the exclusive prefix sum of 1 + D * popcount(mask)");
    sum += step_sel_rows(m, D);
  }
  mask.resize((size_t)n);
  if (mask_out) *mask_out = mask;
  *total = sum;
  return TTX_OK;
}

extern "C" int ttx_debug_attn_select(ttx_session* s, const float* d_q, int ldq, const float* d_k, const float* d_v, int ldkv, float* d_out,
                                     int H, float scale, int Lk, const int32_t* d_tok, int pad, const uint8_t* d_key_pad,
                                     const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_src_of, const int32_t* d_src_len,
                                     const float* d_kcache, const float* d_vcache, int64_t cache_seq_stride, const int32_t* d_cache_slot,
                                     int gen_ld, int N, int D, int mode, int groups, int n_active, int max_keys, int kernel,
                                     int32_t* kernel_id, const int32_t* d_row_base, const int32_t* d_draft_mask, void* stream) {
  if (!s) return fail(TTX_ERR_INVALID, "null session");
  if (mode != ATT_STEP_SELF && mode != ATT_STEP_CROSS) return fail(TTX_ERR_INVALID, "ttx_debug_attn_select: a step mode (3 or 4) is required");
  if (kernel != 0 && kernel != AK_ATTN3 && kernel != AK_ATTN3S)
    return fail(TTX_ERR_INVALID, "ttx_debug_attn_select: draft select runs on k_attn3 (3) or k_attn3s (4); 0 chooses between them");
  if (n_active < 0 || n_active > groups) return fail(TTX_ERR_INVALID, "ttx_debug_attn_select: n_active must lie in [0, groups]");
  HIP_TRY(hipSetDevice(s->m->device));
  if ((d_row_base != nullptr) != (d_draft_mask != nullptr))
    return fail(TTX_ERR_INVALID, "ttx_debug_attn_select: row_base and draft_mask come together");
  int total = 0;
  if (d_row_base)
    TTX_TRY(dbg_check_select("ttx_debug_attn_select", d_row_base, d_draft_mask, n_active, N, D, reinterpret_cast<hipStream_t>(stream), nullptr, &total));
  AttnArgs a{};
  a.q = d_q; a.ldq = ldq; a.k = d_k; a.v = d_v; a.ldkv = ldkv; a.out = d_out; a.scale = scale; a.Lk = Lk;
  a.tok = d_tok; a.pad = pad; a.key_pad = d_key_pad; a.act_idx = d_act_idx; a.front = d_front;
  a.src_of = d_src_of; a.src_len = d_src_len; a.kcache = d_kcache; a.vcache = d_vcache; a.cache_seq_stride = (long long)cache_seq_stride;
  a.cache_slot = d_cache_slot; a.gen_ld = gen_ld; a.N = N; a.D = D; a.row_base = d_row_base; a.draft_mask = d_draft_mask;
  return attn_debug(s, a, H, 32, mode, groups, n_active, max_keys, kernel, kernel_id, reinterpret_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------
// Test entry points of the loop kernels (tests/test_gpu_loop_kernels.py): ONE launch of k_argmax, k_embed, k_accept /
// k_greedy_accept or k_kvcopy with production's grid and block rules on the caller's device operands.  What the kernels take on
// trust from the production call sites is checked here first, the device-side index arrays included (they are read back: these are
// test calls), so that a test cannot launch a kernel on arguments that would take it out of its operands.
static bool dbg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool dbg_model_d(int d) { return d == 64 || d == 128 || d == 256 || d == 512 || d == 1024; }

// The running list and the fronts of a step launch: act_idx[0, n_active) are distinct rows of [0, B) and every running row leaves
// front + D + 2 <= gen_ld columns (what a verify step reads and writes).  Hands back the largest running front.
static int dbg_check_slots(const char* who, const int32_t* d_act_idx, const int32_t* d_front, int B, int n_active, int gen_ld, int D,
                           hipStream_t st, int* max_front) {
  *max_front = 0;
  if (n_active == 0) return TTX_OK;
  std::vector<int32_t> act((size_t)n_active), front((size_t)B);
  HIP_TRY(hipStreamSynchronize(st));               // the caller's writes are ordered on its stream
  HIP_TRY(hipMemcpy(act.data(), d_act_idx, (size_t)n_active * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(front.data(), d_front, (size_t)B * 4, hipMemcpyDeviceToHost));
  std::vector<char> seen((size_t)B, 0);
  for (int i = 0; i < n_active; ++i) {
    const int b = act[i];
    if (b < 0 || b >= B || seen[b]) return fail(TTX_ERR_INVALID, std::string(who) + ": act_idx must hold distinct rows of [0, B)");
    seen[b] = 1;
    if (front[b] < 0 || (long long)front[b] + D + 2 > gen_ld)
      return fail(TTX_ERR_INVALID, std::string(who) + ": gen_ld is too small for front + D + 2 (or a front is negative)");
    *max_front = std::max(*max_front, (int)front[b]);
  }
  return TTX_OK;
}

// ONE launch of k_logit_bias on the caller's device arrays (tests/test_gpu_logit_bias_kernel.py): the plain mapping (d_act_idx null:
// d_src by row, or null for row / rows_per_src) or the step layout (d_act_idx set: d_row_map or null, N, D).
extern "C" int ttx_debug_logit_bias(ttx_session* s, float* d_logits, int V, int M, const int32_t* d_m, const float* d_bias, int ld_bias,
                                    const int32_t* d_src, int rows_per_src, const int32_t* d_act_idx, const int32_t* d_row_map, int N, int D,
                                    void* stream) {
  if (!s) return session_required("ttx_debug_logit_bias");
  if (!d_logits || !d_bias || V <= 0 || M <= 0 || ld_bias < V) return fail(TTX_ERR_INVALID, "bad argument to ttx_debug_logit_bias");
  if (d_act_idx ? (!d_src || N < 1 || D < 0) : (!d_src && rows_per_src < 1))
    return fail(TTX_ERR_INVALID, "ttx_debug_logit_bias: the step layout needs d_src, N >= 1 and D >= 0; the plain mapping d_src or rows_per_src >= 1");
  HIP_TRY(hipSetDevice(s->m->device));
  LogitBiasArgs a{};
  a.logits = d_logits; a.V = V; a.m_ptr = d_m; a.M = M; a.tab = LogitBiasTab{d_bias, ld_bias, d_src}; a.rows_per_src = std::max(rows_per_src, 1);
  a.act_idx = d_act_idx; a.row_map = d_row_map; a.N = N; a.D = D;
  return launch_logit_bias((hipStream_t)stream, a, d_act_idx != nullptr);
}

// k_logit_bias launches the session has enqueued (eagerly or into a captured step; a replayed graph adds none) since it was created,
// ttx_debug_logit_bias's not counted: 0 for a session that never served a biased call.
extern "C" int ttx_debug_logit_bias_launches(ttx_session* s) {
  return s ? (int)std::min<long long>(s->logit_bias_launches, 0x7fffffff) : 0;
}

// ONE launch of k_syntax_mask on the caller's device arrays (tests/test_gpu_syntax_kernel.py).  mode 0: the plain mapping (d_tok int32
// [M][ld_tok], d_front one int); 1: the step layout (d_tok int32 [B][ld_tok], d_front [B], d_act_idx, d_row_map or null, d_drafts
// [B][N][D]); 2: teacher-forced (d_tok int64 [M / T][ld_tok], rows of T positions).  Every index is the caller's to keep in range.
extern "C" int ttx_debug_syntax_mask(ttx_session* s, int mode, float* d_logits, int V, int M, const int32_t* d_m, const int8_t* d_cls,
                                     int max_len, int eos, const void* d_tok, int ld_tok, const int32_t* d_front,
                                     const int32_t* d_act_idx, const int32_t* d_row_map, const int32_t* d_drafts, int N, int D, int T,
                                     void* stream) {
  if (!s) return session_required("ttx_debug_syntax_mask");
  if (!d_logits || !d_cls || !d_tok || V <= 0 || M <= 0 || ld_tok < 1 || mode < 0 || mode > 2)
    return fail(TTX_ERR_INVALID, "bad argument to ttx_debug_syntax_mask");
  if (mode == 1 ? (!d_front || !d_act_idx || N < 1 || D < 0 || (D > 0 && !d_drafts)) : mode == 0 ? !d_front : (T < 1 || M % T != 0 || ld_tok <= T - 1))
    return fail(TTX_ERR_INVALID, "ttx_debug_syntax_mask: the step layout needs d_front, d_act_idx, N >= 1, D >= 0 and drafts; the plain "
                                 "mapping d_front; the teacher-forced one T >= 1, M a multiple of T and ld_tok >= T");
  HIP_TRY(hipSetDevice(s->m->device));
  SyntaxArgs a{};
  a.logits = d_logits; a.V = V; a.m_ptr = d_m; a.M = M; a.cls = reinterpret_cast<const signed char*>(d_cls); a.max_len = max_len; a.eos = eos;
  if (mode == 2) { a.hyp = static_cast<const int64_t*>(d_tok); a.ld_hyp = ld_tok; a.T = T; }
  else { a.gen = static_cast<const int*>(d_tok); a.gen_ld = ld_tok; a.front = d_front; }
  if (mode == 1) { a.act_idx = d_act_idx; a.row_map = d_row_map; a.drafts = d_drafts; a.N = N; a.D = D; }
  return launch_syntax_mask((hipStream_t)stream, a, mode == 1);
}

// k_syntax_mask launches the session has enqueued (eagerly or into a captured step; a replayed graph adds none) since it was created,
// ttx_debug_syntax_mask's not counted: 0 for a session that never served a constrained call.
extern "C" int ttx_debug_syntax_launches(ttx_session* s) {
  return s ? (int)std::min<long long>(s->syntax_launches, 0x7fffffff) : 0;
}

extern "C" int ttx_debug_argmax(ttx_session* s, const float* d_logits, int V, int32_t* d_pred, const int32_t* d_m, int m_max,
                                void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !d_logits || !d_pred) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_argmax");
  if (V < 1 || m_max < 1) return fail(TTX_ERR_INVALID, "ttx_debug_argmax: V and m_max must be positive");
  HIP_TRY(hipSetDevice(s->m->device));
  if (d_m) {
    int32_t m = -1;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(&m, d_m, 4, hipMemcpyDeviceToHost));
    if (m < 0 || m > m_max) return fail(TTX_ERR_INVALID, "ttx_debug_argmax: the live row count on the device is outside [0, m_max]");
  }
  hipLaunchKernelGGL(k_argmax, dim3(cdiv(m_max, 4)), dim3(256), 0, st, d_logits, V, d_pred, d_m, m_max);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

// The prefix table of a debug launch over `rows` decoder rows, checked on the host: every row's source inside the table, every
// length in [0, ld].  The caller's writes are ordered on its stream.
static int dbg_prefix_tab(const char* who, const ttx_debug_prefix* x, int rows, hipStream_t st, PrefixTab* out) {
  if (!x || !x->d_tok || !x->d_len || !x->d_src || x->ld < 1 || x->n_sources < 1)
    return fail(TTX_ERR_INVALID, std::string(who) + ": the prefix table needs d_tok, d_len, d_src, ld >= 1 and n_sources >= 1");
  std::vector<int32_t> len((size_t)rows), src((size_t)rows);
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(len.data(), x->d_len, (size_t)rows * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(src.data(), x->d_src, (size_t)rows * 4, hipMemcpyDeviceToHost));
  for (int r = 0; r < rows; ++r)
    if (len[r] < 0 || len[r] > x->ld || src[r] < 0 || src[r] >= x->n_sources)
      return fail(TTX_ERR_INVALID, std::string(who) + ": a prefix length lies outside [0, ld] or a source outside the table");
  *out = PrefixTab{x->d_tok, x->ld, x->d_len, x->d_src};
  return TTX_OK;
}

static int sample_debug(const char* who_c, ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample,
                        int32_t* d_done, const int32_t* d_front, int32_t* d_pred, const int32_t* d_m, int m_max,
                        const ttx_sample_params* p, const ttx_debug_prefix* pfx, bool prompted, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !d_logits || !d_key || !d_sample || !d_done || !d_front || !d_pred || !p)
    return fail(TTX_ERR_INVALID, "null argument to ttx_debug_sample");
  if (V < 1 || V > SAMPLE_MAX_V || m_max < 1) return fail(TTX_ERR_INVALID, "ttx_debug_sample: V must be in [1, 1024] and m_max positive");
  SampleBlock blk{};
  TTX_TRY(sample_block("ttx_debug_sample", p, &blk));
  HIP_TRY(hipSetDevice(s->m->device));
  if (d_m) {
    int32_t m = -1;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(&m, d_m, 4, hipMemcpyDeviceToHost));
    if (m < 0 || m > m_max) return fail(TTX_ERR_INVALID, "ttx_debug_sample: the live row count on the device is outside [0, m_max]");
  }
  TTX_TRY(ensure(s->smp_prm, sizeof(SampleBlock), st));
  hipLaunchKernelGGL(k_sample_params, dim3(1), dim3(64), 0, st, s->smp_prm.as<SampleBlock>(), blk);
  HIP_TRY(hipGetLastError());
  SampleArgs a{};
  a.logits = d_logits; a.V = V; a.pred = d_pred; a.m_ptr = d_m; a.M = m_max;
  a.key = reinterpret_cast<const unsigned long long*>(d_key); a.sample = d_sample; a.done = d_done; a.front = d_front;
  a.prm = s->smp_prm.as<SampleBlock>();
  if (prompted) {
    int32_t f = -1;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(&f, d_front, 4, hipMemcpyDeviceToHost));
    if (f < 0) return fail(TTX_ERR_INVALID, std::string(who_c) + ": the front must not be negative");
    TTX_TRY(dbg_prefix_tab(who_c, pfx, m_max, st, &a.pfx));
  }
  return launch_sample(st, a);
}

extern "C" int ttx_debug_sample(ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample,
                                int32_t* d_done, const int32_t* d_front, int32_t* d_pred, const int32_t* d_m, int m_max,
                                const ttx_sample_params* p, void* stream) {
  return sample_debug("ttx_debug_sample", s, d_logits, V, d_key, d_sample, d_done, d_front, d_pred, d_m, m_max, p, nullptr, false, stream);
}

extern "C" int ttx_debug_sample_prefix(ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample,
                                       int32_t* d_done, const int32_t* d_front, int32_t* d_pred, const int32_t* d_m, int m_max,
                                       const ttx_sample_params* p, const ttx_debug_prefix* pfx, void* stream) {
  return sample_debug("ttx_debug_sample_prefix", s, d_logits, V, d_key, d_sample, d_done, d_front, d_pred, d_m, m_max, p, pfx, true, stream);
}

// `select` (ttx_debug_sample_step_select): the launch covers n_rows rows stored compacted, row i drawing for layout row d_row_map[i]
// (null: row i itself), and the probe layout N = 1, D = 0 is accepted.
static int sample_step_debug(const char* who_c, ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample,
                             const int32_t* d_act_idx, const int32_t* d_front, int B, int N, int D, int n_active, int32_t* d_pred,
                             const int32_t* d_m, const ttx_sample_params* p, void* stream, bool select, const int32_t* d_row_map,
                             int n_rows, const ttx_debug_prefix* pfx = nullptr, bool prompted = false) {
  const std::string who(who_c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !d_logits || !d_key || !d_sample || !d_act_idx || !d_front || !d_pred || !p)
    return fail(TTX_ERR_INVALID, "null argument to " + who);
  if (V < 1 || V > SAMPLE_MAX_V) return fail(TTX_ERR_INVALID, who + ": V must be in [1, 1024]");
  const bool probe = select && N == 1 && D == 0;
  if (B < 1 || N < 1 || (D < 1 && !probe) || (long long)B * step_rps(N, D) * V >= (1ll << 31))
    return fail(TTX_ERR_INVALID, who + ": B, N and D must be positive and the logits below 2^31 elements");
  if (n_active < 0 || n_active > B) return fail(TTX_ERR_INVALID, who + ": n_active must lie in [0, B]");
  if (!select && !d_m && n_active != B) return fail(TTX_ERR_INVALID, who + ": without a live row count every slot must be active");
  const int RPS = step_rps(N, D);
  if (select && (n_rows < 1 || n_rows > n_active * RPS)) return fail(TTX_ERR_INVALID, who + ": n_rows must lie in [1, n_active * (1 + N*D)]");
  if (select && !d_row_map && n_rows != n_active * RPS) return fail(TTX_ERR_INVALID, who + ": without a row map the launch covers every row of the active slots");
  SampleBlock blk{};
  TTX_TRY(sample_block(who_c, p, &blk));
  HIP_TRY(hipSetDevice(s->m->device));
  int max_front = 0;
  TTX_TRY(dbg_check_slots(who_c, d_act_idx, d_front, B, n_active, 1 << 30, D, st, &max_front));
  const int M = select ? n_rows : B * RPS;
  if (d_m) {
    int32_t m = -1;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(&m, d_m, 4, hipMemcpyDeviceToHost));
    if (m < 0 || m > (select ? n_rows : n_active * RPS)) return fail(TTX_ERR_INVALID, who + ": the live row count on the device is outside the launch's rows");
  }
  if (d_row_map) {
    std::vector<int32_t> map((size_t)n_rows);
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(map.data(), d_row_map, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
    for (const int32_t r : map)
      if (r < 0 || r >= n_active * RPS) return fail(TTX_ERR_INVALID, who + ": a row map entry lies outside the active slots' rows");
  }
  TTX_TRY(ensure(s->smp_prm, sizeof(SampleBlock), st));
  hipLaunchKernelGGL(k_sample_params, dim3(1), dim3(64), 0, st, s->smp_prm.as<SampleBlock>(), blk);
  HIP_TRY(hipGetLastError());
  SampleStepArgs a{};
  a.logits = d_logits; a.V = V; a.pred = d_pred; a.m_ptr = d_m; a.M = M;
  a.key = reinterpret_cast<const unsigned long long*>(d_key); a.sample = d_sample; a.act_idx = d_act_idx; a.front = d_front;
  a.N = N; a.D = D; a.prm = s->smp_prm.as<SampleBlock>(); a.row_map = d_row_map;
  if (prompted) TTX_TRY(dbg_prefix_tab(who_c, pfx, B, st, &a.pfx));
  return launch_sample_step(st, a);
}

extern "C" int ttx_debug_sample_step(ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample,
                                     const int32_t* d_act_idx, const int32_t* d_front, int B, int N, int D, int n_active,
                                     int32_t* d_pred, const int32_t* d_m, const ttx_sample_params* p, void* stream) {
  return sample_step_debug("ttx_debug_sample_step", s, d_logits, V, d_key, d_sample, d_act_idx, d_front, B, N, D, n_active, d_pred, d_m, p,
                           stream, false, nullptr, 0);
}

extern "C" int ttx_debug_sample_step_select(ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample,
                                            const int32_t* d_act_idx, const int32_t* d_front, int B, int N, int D, int n_active,
                                            int32_t* d_pred, const int32_t* d_m, const ttx_sample_params* p, const int32_t* d_row_map,
                                            int n_rows, void* stream) {
  return sample_step_debug("ttx_debug_sample_step_select", s, d_logits, V, d_key, d_sample, d_act_idx, d_front, B, N, D, n_active, d_pred,
                           d_m, p, stream, true, d_row_map, n_rows);
}

extern "C" int ttx_debug_sample_step_prefix(ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample,
                                            const int32_t* d_act_idx, const int32_t* d_front, int B, int N, int D, int n_active,
                                            int32_t* d_pred, const int32_t* d_m, const ttx_sample_params* p, const int32_t* d_row_map,
                                            int n_rows, const ttx_debug_prefix* pfx, void* stream) {
  return sample_step_debug("ttx_debug_sample_step_prefix", s, d_logits, V, d_key, d_sample, d_act_idx, d_front, B, N, D, n_active, d_pred,
                           d_m, p, stream, true, d_row_map, n_rows, pfx, true);
}

extern "C" int ttx_debug_prefix_drafts(ttx_session* s, const int32_t* d_act_idx, const int32_t* d_front, int B, int N, int D, int n_active,
                                       int32_t* d_drafts, const int32_t* d_draft0, const ttx_debug_prefix* pfx, int eos_token,
                                       int pad_token, int replace_token, void* stream) {
  const char* who = "ttx_debug_prefix_drafts";
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !d_act_idx || !d_front || !d_drafts || !d_draft0) return fail(TTX_ERR_INVALID, std::string("null argument to ") + who);
  if (B < 1 || N < 1 || D < 1 || (long long)B * N * D >= (1ll << 31)) return fail(TTX_ERR_INVALID, std::string(who) + ": B, N and D must be positive");
  if (n_active < 0 || n_active > B) return fail(TTX_ERR_INVALID, std::string(who) + ": n_active must lie in [0, B]");
  HIP_TRY(hipSetDevice(s->m->device));
  int max_front = 0;
  TTX_TRY(dbg_check_slots(who, d_act_idx, d_front, B, n_active, 1 << 30, D, st, &max_front));
  PrefixDraftsArgs a{};
  TTX_TRY(dbg_prefix_tab(who, pfx, B, st, &a.pfx));
  DecState* dst = nullptr;
  HIP_TRY(hipMalloc((void**)&dst, sizeof(DecState)));
  DecState hs{};
  hs.n_active = n_active; hs.r_rows = n_active * N; hs.m_rows = n_active * step_rps(N, D);
  hipError_t err = hipMemcpy(dst, &hs, sizeof(DecState), hipMemcpyHostToDevice);
  int rc = TTX_OK;
  if (err == hipSuccess) {
    a.st = dst; a.act_idx = d_act_idx; a.front = d_front; a.drafts = d_drafts; a.N = N; a.D = D; a.draft0 = d_draft0;
    a.eos = eos_token; a.pad = pad_token; a.repl = replace_token;
    rc = launch_prefix_drafts_args(st, a, B);         // production's grid: one wave per slot of the capacity
  }
  const hipError_t esync = hipStreamSynchronize(st);   // the launch reads the state: keep it until the launch is through
  (void)hipFree(dst);
  HIP_TRY(err);
  HIP_TRY(esync);
  return rc;
}

extern "C" int ttx_debug_proposal_drafts(ttx_session* s, const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_gen, int gen_ld,
                                         int B, int N, int D, int n_active, int32_t* d_drafts, const int32_t* d_draft0,
                                         const ttx_debug_prefix* proposal, int ctx, int bos_token, int eos_token, int pad_token,
                                         int replace_token, void* stream) {
  const char* who = "ttx_debug_proposal_drafts";
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !d_act_idx || !d_front || !d_gen || !d_drafts || !d_draft0) return fail(TTX_ERR_INVALID, std::string("null argument to ") + who);
  if (B < 1 || N < 1 || D < 1 || gen_ld < 1 || (long long)B * N * D >= (1ll << 31) || (long long)B * gen_ld >= (1ll << 31))
    return fail(TTX_ERR_INVALID, std::string(who) + ": B, N, D and gen_ld must be positive");
  if (n_active < 0 || n_active > B) return fail(TTX_ERR_INVALID, std::string(who) + ": n_active must lie in [0, B]");
  if (ctx != 2 && ctx != 4 && ctx != 8) return fail(TTX_ERR_INVALID, std::string(who) + ": ctx must be 2, 4 or 8");
  HIP_TRY(hipSetDevice(s->m->device));
  int max_front = 0;
  // the kernel reads gen[0 .. front] of the active rows: front + 1 <= gen_ld (dbg_check_slots asks for front + 0 + 2)
  TTX_TRY(dbg_check_slots(who, d_act_idx, d_front, B, n_active, gen_ld + 1, 0, st, &max_front));
  ProposalDraftsArgs a{};
  TTX_TRY(dbg_prefix_tab(who, proposal, B, st, &a.tab));
  DecState* dst = nullptr;
  HIP_TRY(hipMalloc((void**)&dst, sizeof(DecState)));
  DecState hs{};
  hs.n_active = n_active; hs.r_rows = n_active * N; hs.m_rows = n_active * step_rps(N, D);
  hipError_t err = hipMemcpy(dst, &hs, sizeof(DecState), hipMemcpyHostToDevice);
  int rc = TTX_OK;
  if (err == hipSuccess) {
    a.st = dst; a.act_idx = d_act_idx; a.front = d_front; a.gen = d_gen; a.gen_ld = gen_ld; a.drafts = d_drafts; a.N = N; a.D = D;
    a.draft0 = d_draft0; a.bos = bos_token; a.eos = eos_token; a.pad = pad_token; a.repl = replace_token; a.ctx = ctx;
    rc = launch_proposal_drafts_args(st, a, B);       // production's grid: one wave per slot of the capacity
  }
  const hipError_t esync = hipStreamSynchronize(st);   // the launch reads the state: keep it until the launch is through
  (void)hipFree(dst);
  HIP_TRY(err);
  HIP_TRY(esync);
  return rc;
}

// d_row_map (ttx_debug_embed_select; null: ttx_debug_embed): the launch writes m_rows rows, row i holding layout row d_row_map[i]
static int embed_debug(ttx_session* s, const float* d_table, int V, const float* d_pe, int pe_rows, int d, float* d_x,
                       const int32_t* d_tok, int rows, int L, const int32_t* d_act_idx, const int32_t* d_front,
                       const int32_t* d_gen, int gen_ld, const int32_t* d_drafts, int B, int N, int D, int n_active, int step,
                       const int32_t* d_row_map, int m_rows, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !d_table || !d_pe || !d_x) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_embed");
  if (!dbg_model_d(d)) return fail(TTX_ERR_INVALID, "ttx_debug_embed: d must be 64, 128, 256, 512 or 1024");
  if (V < 1 || pe_rows < 1) return fail(TTX_ERR_INVALID, "ttx_debug_embed: V and pe_rows must be positive");
  if (!dbg_aligned16(d_table) || !dbg_aligned16(d_pe) || !dbg_aligned16(d_x))
    return fail(TTX_ERR_INVALID, "ttx_debug_embed: float operands must be 16-byte aligned");
  HIP_TRY(hipSetDevice(s->m->device));
  EmbedArgs e{};
  e.table = d_table; e.pe = d_pe; e.X = d_x; e.d = d; e.V = V;
  if (!step) {
    if (!d_tok || rows < 1 || L < 1) return fail(TTX_ERR_INVALID, "ttx_debug_embed: full mode needs tokens, rows >= 1 and L >= 1");
    if (pe_rows < L + 1) return fail(TTX_ERR_INVALID, "ttx_debug_embed: the positional table must have L + 1 rows");
    e.tok = d_tok; e.rows = rows; e.L = L;
    hipLaunchKernelGGL((k_embed<false>), dim3(cdiv(rows, 4)), dim3(256), 0, st, e);
    HIP_TRY(hipGetLastError());
    return TTX_OK;
  }
  if (!d_act_idx || !d_front || !d_gen || !d_drafts) return fail(TTX_ERR_INVALID, "ttx_debug_embed: step mode needs act_idx, front, gen and drafts");
  if (B < 1 || N < 1 || D < 1 || gen_ld < 1) return fail(TTX_ERR_INVALID, "ttx_debug_embed: step mode needs B, N, D and gen_ld >= 1");
  if (n_active < 0 || n_active > B) return fail(TTX_ERR_INVALID, "ttx_debug_embed: n_active must lie in [0, B]");
  int max_front = 0;
  TTX_TRY(dbg_check_slots("ttx_debug_embed", d_act_idx, d_front, B, n_active, gen_ld, D, st, &max_front));
  if (n_active > 0 && pe_rows < max_front + D + 2) return fail(TTX_ERR_INVALID, "ttx_debug_embed: the positional table must have front + D + 2 rows");
  const int RPS = step_rps(N, D);
  if (d_row_map) {
    if (m_rows < 0 || m_rows > n_active * RPS) return fail(TTX_ERR_INVALID, "ttx_debug_embed_select: m_rows must lie in [0, n_active * (1 + N*D)]");
    std::vector<int32_t> map((size_t)std::max(m_rows, 1));
    HIP_TRY(hipStreamSynchronize(st));
    if (m_rows > 0) HIP_TRY(hipMemcpy(map.data(), d_row_map, (size_t)m_rows * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < m_rows; ++i)
      if (map[i] < 0 || map[i] >= n_active * RPS) return fail(TTX_ERR_INVALID, "ttx_debug_embed_select: row_map must hold layout rows of the live slots");
  }
  // the live row count reaches the kernel as production hands it over: in a DecState on the device, written on the launch's stream
  DecState* dst = nullptr;
  HIP_TRY(hipMalloc((void**)&dst, sizeof(DecState)));
  DecState* hs = reinterpret_cast<DecState*>(s->host_state);
  *hs = DecState{};
  hs->n_active = n_active; hs->r_rows = n_active * N; hs->m_rows = d_row_map ? m_rows : n_active * RPS;
  hipError_t err = hipMemcpyAsync(dst, hs, sizeof(DecState), hipMemcpyHostToDevice, st);
  if (err == hipSuccess) {
    e.st = dst; e.act_idx = d_act_idx; e.front = d_front; e.gen = d_gen; e.gen_ld = gen_ld; e.drafts = d_drafts; e.N = N; e.D = D;
    e.row_map = d_row_map;
    hipLaunchKernelGGL((k_embed<true>), dim3(cdiv(B * RPS, 4)), dim3(256), 0, st, e);
    err = hipGetLastError();
  }
  const hipError_t esync = hipStreamSynchronize(st);   // the launch reads the state: keep it until the launch is through
  (void)hipFree(dst);
  HIP_TRY(err);
  HIP_TRY(esync);
  return TTX_OK;
}

extern "C" int ttx_debug_embed(ttx_session* s, const float* d_table, int V, const float* d_pe, int pe_rows, int d, float* d_x,
                               const int32_t* d_tok, int rows, int L, const int32_t* d_act_idx, const int32_t* d_front,
                               const int32_t* d_gen, int gen_ld, const int32_t* d_drafts, int B, int N, int D, int n_active, int step,
                               void* stream) {
  return embed_debug(s, d_table, V, d_pe, pe_rows, d, d_x, d_tok, rows, L, d_act_idx, d_front, d_gen, gen_ld, d_drafts, B, N, D, n_active,
                     step, nullptr, 0, stream);
}

extern "C" int ttx_debug_embed_select(ttx_session* s, const float* d_table, int V, const float* d_pe, int pe_rows, int d, float* d_x,
                                      const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_gen, int gen_ld,
                                      const int32_t* d_drafts, int B, int N, int D, int n_active, const int32_t* d_row_map, int m_rows,
                                      void* stream) {
  return embed_debug(s, d_table, V, d_pe, pe_rows, d, d_x, nullptr, 0, 0, d_act_idx, d_front, d_gen, gen_ld, d_drafts, B, N, D, n_active, 1,
                     d_row_map, m_rows, stream);
}

// ttx_debug_accept; `sample`: ttx_debug_sample_accept, k_sample_accept on the same argument block
// `sample_pool` (ttx_debug_sample_accept_pool): the sampling rule in pool mode (pool = row_rule = 1; the traj / fin_step pointers are
// unused), with the executed-row count at d_exec_rows (may be null) and, with `spread`, the pair k_sample_accept_slots +
// k_accept_finish whatever B is.
static int accept_debug(ttx_session* s, const ttx_debug_accept_args* a, int64_t* state, void* stream, bool sample, bool sample_pool = false,
                        const int32_t* d_exec_rows = nullptr, bool spread = false) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !a || !state) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_accept");
  if (sample_pool && (a->greedy || !a->row_rule || !a->pool))
    return fail(TTX_ERR_INVALID, "ttx_debug_sample_accept_pool: greedy must be 0, row_rule and pool 1");
  if (sample_pool && spread && a->threads != 0) return fail(TTX_ERR_INVALID, "ttx_debug_sample_accept_pool: the pair runs with threads = 0");
  if (sample && !sample_pool && (a->greedy || a->row_rule || a->pool))
    return fail(TTX_ERR_INVALID, "ttx_debug_sample_accept: greedy, row_rule and pool must be 0");
  if (!a->d_act_idx || !a->d_front || !a->d_gen || !a->d_pred || !a->d_rec)
    return fail(TTX_ERR_INVALID, "ttx_debug_accept: act_idx, front, gen, pred and rec are required");
  const bool greedy = a->greedy != 0;
  if (greedy && (a->row_rule || a->pool || a->N != 1 || a->D != 0))
    return fail(TTX_ERR_INVALID, "ttx_debug_accept: plain greedy runs with N = 1, D = 0 and neither row_rule nor pool");
  if (!greedy && (!a->d_drafts || !a->d_haspad || a->N < 1 || a->D < 1))
    return fail(TTX_ERR_INVALID, "ttx_debug_accept: the speculative step needs drafts, haspad, N >= 1 and D >= 1");
  if (a->pool && !a->row_rule) return fail(TTX_ERR_INVALID, "ttx_debug_accept: pool implies row_rule");
  if (!greedy && !a->pool && !a->d_out) return fail(TTX_ERR_INVALID, "ttx_debug_accept: out is required outside pool mode");
  if (a->row_rule && !a->pool && (!a->d_traj || !a->d_fin_step)) return fail(TTX_ERR_INVALID, "ttx_debug_accept: row_rule needs traj and fin_step");
  if (sample_pool && (!a->d_row_of || !a->d_pool_out || a->pool_rows < 1))
    return fail(TTX_ERR_INVALID, "ttx_debug_sample_accept_pool: pool mode needs row_of and the caller-side out rows");
  if (a->pool && !sample_pool && (!a->d_rstep || !a->d_row_of || !a->d_pool_out || !a->d_pool_traj || !a->d_pool_fin_step || a->pool_rows < 1))
    return fail(TTX_ERR_INVALID, "ttx_debug_accept: pool mode needs rstep, row_of and the caller-side out, traj and fin_step rows");
  if (a->row_rule && a->traj_ld < 1) return fail(TTX_ERR_INVALID, "ttx_debug_accept: traj_ld must be positive");
  if (a->B < 1 || a->max_len < 1 || a->gen_ld < 1 || a->Ls < 0) return fail(TTX_ERR_INVALID, "ttx_debug_accept: B, max_len and gen_ld must be positive");
  // production launches 256 threads for B <= 256 and ACCEPT_THREADS above; 256 threads at B > 256 is a launch it never makes
  if (a->threads != 0 && a->threads != 256 && a->threads != ACCEPT_THREADS) return fail(TTX_ERR_INVALID, "ttx_debug_accept: threads is 0, 256 or 1024");
  if (a->threads == 256 && a->B > 256) return fail(TTX_ERR_INVALID, "ttx_debug_accept: 256 threads are never launched for B > 256");
  if (greedy && a->threads == ACCEPT_THREADS) return fail(TTX_ERR_INVALID, "ttx_debug_accept: plain greedy always runs with 256 threads");
  const int n_active = (int)state[0];
  if (state[0] < 0 || state[0] > a->B) return fail(TTX_ERR_INVALID, "ttx_debug_accept: n_active must lie in [0, B]");
  if (a->gen_ld < a->max_len) return fail(TTX_ERR_INVALID, "ttx_debug_accept: gen_ld must cover max_len (finished rows are copied from gen)");
  HIP_TRY(hipSetDevice(s->m->device));
  int max_front = 0;
  if (greedy) {
    // every row shares the front of row 0 and the running rows are rows [0, n_active)
    if (n_active > 0) {
      int32_t f0 = -1;
      HIP_TRY(hipStreamSynchronize(st));
      HIP_TRY(hipMemcpy(&f0, a->d_front, 4, hipMemcpyDeviceToHost));
      if (f0 < 0 || (long long)f0 + 2 > a->gen_ld) return fail(TTX_ERR_INVALID, "ttx_debug_accept: gen_ld is too small for front + D + 2");
    }
  } else {
    TTX_TRY(dbg_check_slots("ttx_debug_accept", a->d_act_idx, a->d_front, a->B, n_active, a->gen_ld, a->D, st, &max_front));
    if (a->pool && n_active > 0) {
      std::vector<int32_t> row_of((size_t)a->B);
      HIP_TRY(hipMemcpy(row_of.data(), a->d_row_of, (size_t)a->B * 4, hipMemcpyDeviceToHost));
      std::vector<int32_t> act((size_t)n_active);
      HIP_TRY(hipMemcpy(act.data(), a->d_act_idx, (size_t)n_active * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < n_active; ++i)
        if (row_of[act[i]] < 0 || row_of[act[i]] >= a->pool_rows) return fail(TTX_ERR_INVALID, "ttx_debug_accept: row_of must lie in [0, pool_rows)");
    }
  }
  HostInfo* hinfo = nullptr;
  HostInfo* dev_info = nullptr;
  DecState* dst = nullptr;
  PoolIo* dio = nullptr;
  hipError_t err = hipHostMalloc((void**)&hinfo, sizeof(HostInfo), hipHostMallocMapped);
  if (err == hipSuccess) err = hipHostGetDevicePointer((void**)&dev_info, (void*)hinfo, 0);
  if (err == hipSuccess) err = hipMalloc((void**)&dst, sizeof(DecState));
  if (err == hipSuccess && a->pool) err = hipMalloc((void**)&dio, sizeof(PoolIo));
  DecState* hs = reinterpret_cast<DecState*>(s->host_state);
  PoolIo hio{a->d_pool_out, a->d_pool_traj, a->d_pool_fin_step, a->traj_ld, 0};
  if (err == hipSuccess) {
    *hinfo = HostInfo{-1, -1, -1, -1};
    hs->n_active = n_active; hs->r_rows = (int)state[1]; hs->m_rows = (int)state[2]; hs->stop = (int)state[3];
    hs->width = (int)state[4]; hs->steps = (int)state[5]; hs->error = (int)state[6]; hs->n_copy = (int)state[7];
    hs->accepted = state[8]; hs->produced = state[9]; hs->verified_positions = state[10]; hs->kv_prefix_positions = state[11];
    hs->src_positions = state[12];
    // the entry state reaches the kernel as production hands it over: in a DecState on the device, written on the launch's stream
    err = hipMemcpyAsync(dst, hs, sizeof(DecState), hipMemcpyHostToDevice, st);
  }
  if (err == hipSuccess && a->pool) err = hipMemcpyAsync(dio, &hio, sizeof(PoolIo), hipMemcpyHostToDevice, st);
  if (err == hipSuccess) {
    LoopArgs la{};
    la.st = dst; la.act_idx = a->d_act_idx; la.front = a->d_front; la.gen = a->d_gen; la.gen_ld = a->gen_ld;
    la.drafts = a->d_drafts; la.pred = a->d_pred; la.rec = reinterpret_cast<CopyRec*>(a->d_rec); la.out = a->d_out;
    la.host = dev_info; la.haspad = a->d_haspad;
    la.row_rule = a->row_rule ? 1 : 0; la.traj = a->d_traj; la.traj_ld = a->traj_ld; la.fin_step = a->d_fin_step;
    la.pool = a->pool ? 1 : 0; la.rstep = a->d_rstep; la.row_of = a->d_row_of; la.io = dio;
    la.B = a->B; la.N = a->N; la.D = a->D; la.Ls = a->Ls; la.max_len = a->max_len; la.pad = a->pad; la.bos = a->bos; la.eos = a->eos;
    // threads = 0 is the production route: above 256 slots the pair, unless TTX_ACCEPT_SPREAD=0
    int rc_blk = TTX_OK;
    la.sample_rule = sample ? 1 : 0;
    la.exec_rows = d_exec_rows;
    if (!greedy && !sample && a->threads == 0) rc_blk = accept_blk_for(s, st, a->B, &la.blk);
    if (sample_pool && spread) {
      const void* before = s->accept_blk.p;
      rc_blk = ensure(s->accept_blk, sizeof(AcceptBlk), st);
      if (rc_blk == TTX_OK && s->accept_blk.p != before && hipMemsetAsync(s->accept_blk.p, 0, sizeof(AcceptBlk), st) != hipSuccess) rc_blk = TTX_ERR_HIP;
      la.blk = s->accept_blk.as<AcceptBlk>();
    }
    if (rc_blk != TTX_OK) err = hipErrorOutOfMemory;
    else if (sample) {
      if (a->threads == 0) { if (launch_sample_accept(st, la) != TTX_OK) err = hipErrorLaunchFailure; }
      else { hipLaunchKernelGGL(k_sample_accept, dim3(1), dim3(a->threads), 0, st, la); err = hipGetLastError(); }
    }
    else if (greedy) { hipLaunchKernelGGL(k_greedy_accept, dim3(1), dim3(256), 0, st, la); err = hipGetLastError(); }
    else if (launch_accept(st, la, a->threads) != TTX_OK) err = hipErrorLaunchFailure;
  }
  if (err == hipSuccess) err = hipMemcpyAsync(hs, dst, sizeof(DecState), hipMemcpyDeviceToHost, st);
  const hipError_t esync = hipStreamSynchronize(st);
  if (err == hipSuccess && esync == hipSuccess) {
    state[0] = hs->n_active; state[1] = hs->r_rows; state[2] = hs->m_rows; state[3] = hs->stop; state[4] = hs->width;
    state[5] = hs->steps; state[6] = hs->error; state[7] = hs->n_copy;
    state[8] = hs->accepted; state[9] = hs->produced; state[10] = hs->verified_positions; state[11] = hs->kv_prefix_positions;
    state[12] = hs->src_positions;
    state[13] = hinfo->stop; state[14] = hinfo->steps_done; state[15] = hinfo->width; state[16] = hinfo->n_active;
  }
  if (dio) (void)hipFree(dio);
  if (dst) (void)hipFree(dst);
  if (hinfo) (void)hipHostFree(hinfo);
  HIP_TRY(err);
  HIP_TRY(esync);
  return TTX_OK;
}

extern "C" int ttx_debug_accept(ttx_session* s, const ttx_debug_accept_args* a, int64_t* state, void* stream) {
  return accept_debug(s, a, state, stream, false);
}

extern "C" int ttx_debug_sample_accept(ttx_session* s, const ttx_debug_accept_args* a, int64_t* state, void* stream) {
  return accept_debug(s, a, state, stream, true);
}

extern "C" int ttx_debug_sample_accept_pool(ttx_session* s, const ttx_debug_accept_args* a, int64_t* state, const int32_t* d_exec_rows,
                                            int spread, void* stream) {
  return accept_debug(s, a, state, stream, true, true, d_exec_rows, spread != 0);
}

// One admission of the sampling pool (k_pool_admit, then k_pool_fill unless the admission failed) on the caller's arrays.
extern "C" int ttx_debug_pool_fill_sample(ttx_session* s, const ttx_debug_pool_fill_args* a, int32_t* result, void* stream) {
  const std::string who = "ttx_debug_pool_fill_sample";
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !a || !result) return fail(TTX_ERR_INVALID, "null argument to " + who);
  if (!a->d_act_idx || !a->d_front || !a->d_haspad || !a->d_rstep || !a->d_row_of || !a->d_src_len || !a->d_key || !a->d_sample ||
      !a->d_gen || !a->d_drafts || !a->d_drafts_new || !a->d_src_valid || !a->d_valid_new || !a->d_memkv || !a->d_memkv_new || !a->d_out)
    return fail(TTX_ERR_INVALID, who + ": every array but row_keys is required");
  if (a->B < 1 || a->B > 4096 || a->N < 1 || a->D < 1 || a->n_sources < 1 || a->per_src < 1 || a->first_src < 0 || a->max_len < 1 ||
      a->gen_ld < 1 || a->Ls_new < 1 || a->Ls_cap < a->Ls_new || a->kv_row < 4 || a->kv_row % 4 != 0 || a->out_rows < 1)
    return fail(TTX_ERR_INVALID, who + ": sizes must be positive, Ls_new <= Ls_cap, kv_row a multiple of 4, B at most 4096");
  if (a->n_active < 0 || a->n_active > a->B) return fail(TTX_ERR_INVALID, who + ": n_active must lie in [0, B]");
  const long long rows = (long long)a->n_sources * a->per_src;
  if (rows > 4096) return fail(TTX_ERR_INVALID, who + ": at most 4096 rows per admission");
  if (((long long)a->first_src + a->n_sources) * a->per_src > a->out_rows) return fail(TTX_ERR_INVALID, who + ": the admitted rows lie beyond the caller's out rows");
  if (!dbg_aligned16(a->d_memkv) || !dbg_aligned16(a->d_memkv_new)) return fail(TTX_ERR_INVALID, who + ": the cross K/V arrays must be 16-byte aligned");
  HIP_TRY(hipSetDevice(s->m->device));
  HIP_TRY(hipStreamSynchronize(st));
  if (a->n_active > 0) {
    std::vector<int32_t> act((size_t)a->n_active);
    HIP_TRY(hipMemcpy(act.data(), a->d_act_idx, (size_t)a->n_active * 4, hipMemcpyDeviceToHost));
    std::vector<char> seen((size_t)a->B, 0);
    for (const int32_t b : act) {
      if (b < 0 || b >= a->B || seen[b]) return fail(TTX_ERR_INVALID, who + ": act_idx must hold distinct slots in [0, B)");
      seen[b] = 1;
    }
  }
  DecState* dst = nullptr;
  int32_t* d_new_slot = nullptr;
  HostInfo* hinfo = nullptr;
  HostInfo* dev_info = nullptr;
  hipError_t err = hipMalloc((void**)&dst, sizeof(DecState));
  if (err == hipSuccess) err = hipMalloc((void**)&d_new_slot, (size_t)rows * 4);
  if (err == hipSuccess) err = hipHostMalloc((void**)&hinfo, sizeof(HostInfo), hipHostMallocMapped);
  if (err == hipSuccess) err = hipHostGetDevicePointer((void**)&dev_info, (void*)hinfo, 0);
  DecState hs{};
  hs.n_active = a->n_active; hs.r_rows = a->n_active * a->N; hs.m_rows = a->n_active * step_rps(a->N, a->D); hs.width = 1;
  if (err == hipSuccess) err = hipMemcpy(dst, &hs, sizeof(DecState), hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    *hinfo = HostInfo{-1, -1, -1, -1};
    PoolAdmitArgs pa{};
    pa.st = dst; pa.act_idx = a->d_act_idx; pa.front = a->d_front; pa.haspad = a->d_haspad; pa.rstep = a->d_rstep; pa.row_of = a->d_row_of;
    pa.src_len = a->d_src_len; pa.new_slot = d_new_slot; pa.host = dev_info; pa.B = a->B; pa.N = a->N; pa.D = a->D; pa.R = (int)rows;
    pa.first_row = a->first_src * a->per_src; pa.Ls_new = a->Ls_new;
    pa.key = reinterpret_cast<unsigned long long*>(a->d_key); pa.sample = a->d_sample; pa.row_keys = a->d_row_keys;
    pa.per_src = a->per_src; pa.first_src = a->first_src;
    hipLaunchKernelGGL(k_pool_admit, dim3(1), dim3(256), (size_t)a->B * 4, st, pa);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err == hipSuccess) err = hipMemcpy(&hs, dst, sizeof(DecState), hipMemcpyDeviceToHost);
  if (err == hipSuccess && hs.error == 0) {          // a failed admission handed out fewer slots than rows: nothing to fill
    PoolFillArgs f{};
    f.new_slot = d_new_slot; f.R = (int)rows; f.gen = a->d_gen; f.gen_ld = a->gen_ld; f.bos = a->bos; f.pad = a->pad;
    f.drafts = a->d_drafts; f.drafts_new = a->d_drafts_new; f.nd = a->N * a->D;
    f.src_valid = a->d_src_valid; f.valid_new = a->d_valid_new; f.Ls_cap = a->Ls_cap; f.Ls_new = a->Ls_new;
    f.memkv = a->d_memkv; f.memkv_new = a->d_memkv_new; f.kv_row = a->kv_row;
    f.out_rows = a->d_out; f.max_len = a->max_len; f.traj_ld = a->max_len + 1; f.first_row = a->first_src * a->per_src;
    f.per_src = a->per_src;
    hipLaunchKernelGGL(k_pool_fill, dim3((int)rows, 1 + a->Ls_new), dim3(256), 0, st, f);
    err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(st);
  }
  if (err == hipSuccess) { result[0] = hs.n_active; result[1] = hs.m_rows; result[2] = hs.error; result[3] = hinfo->n_active; }
  if (d_new_slot) (void)hipFree(d_new_slot);
  if (dst) (void)hipFree(dst);
  if (hinfo) (void)hipHostFree(hinfo);
  HIP_TRY(err);
  return TTX_OK;
}

extern "C" int ttx_debug_accept_block(ttx_session* s, int32_t* words, int n_words, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !words || n_words < 0 || (size_t)n_words * 4 > sizeof(AcceptBlk))
    return fail(TTX_ERR_INVALID, "ttx_debug_accept_block: words must hold at most the block's int32 words");
  if (!s->accept_blk.p) return fail(TTX_ERR_INVALID, "ttx_debug_accept_block: this session has not run the accept pair yet");
  HIP_TRY(hipSetDevice(s->m->device));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(words, s->accept_blk.p, (size_t)n_words * 4, hipMemcpyDeviceToHost));
  return TTX_OK;
}

// ---- the beam family, one launch each: the caller's operands through the launch_* halves of the enqueue_* helpers -------------
// Limits the generators enforce before they launch any of these (beam_check_params, beam_start, bsearch_start).
static int dbg_beam_limits(const char* who, int K, int N, int V, int dl) {
  const std::string w(who);
  if (K < 1 || K > NUC_MAX_KEEP) return fail(TTX_ERR_INVALID, w + ": n_best must lie in [1, 32]");
  if (N < 1 || N > BS_MAX_SLOTS) return fail(TTX_ERR_INVALID, w + ": n_drafts must lie in [1, 64]");
  if (V < 1 || V > 64 * NUC_VPL) return fail(TTX_ERR_INVALID, w + ": V must lie in [1, 1024]");
  if (dl < 0 || (size_t)K * (dl + 1) > 1023) return fail(TTX_ERR_INVALID, w + ": dl >= 0 and K * (dl + 1) <= 1023 segments");
  return TTX_OK;
}

static int dbg_vpl(const char* who, int vpl, int V) {
  if (vpl != 0 && vpl != 4 && vpl != 8 && vpl != NUC_VPL) return fail(TTX_ERR_INVALID, std::string(who) + ": vpl is 0, 4, 8 or 16");
  if (vpl != 0 && 64 * vpl < V) return fail(TTX_ERR_INVALID, std::string(who) + ": vpl does not cover V");
  return TTX_OK;
}

static int dbg_launched(int rc, hipStream_t st) {
  const hipError_t e = hipStreamSynchronize(st);
  TTX_TRY(rc);
  HIP_TRY(e);
  return TTX_OK;
}

extern "C" int ttx_debug_bs_prep(ttx_session* s, const ttx_debug_bs_prep_args* a, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !a) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_bs_prep");
  if (!a->d_cand_next || !a->d_len_next || !a->d_fin_next || !a->d_logp_next || !a->d_gen || !a->d_front || !a->d_len || !a->d_active ||
      !a->d_finished || !a->d_logp || !a->d_per_cand || !a->d_drafts32 || (a->smart ? !a->d_lib : !a->d_drafts_all))
    return fail(TTX_ERR_INVALID, "ttx_debug_bs_prep: a required array is null");
  if (a->max_cand < 1 || a->n_cand < 0 || a->n_cand > a->max_cand || a->beam < 1 || a->ld < 1)
    return fail(TTX_ERR_INVALID, "ttx_debug_bs_prep: max_cand, beam and ld must be positive and n_cand in [0, max_cand]");
  if (a->N < 1 || a->N > BS_MAX_SLOTS || a->dl < 0) return fail(TTX_ERR_INVALID, "ttx_debug_bs_prep: N must lie in [1, 64] and dl >= 0");
  if (!a->smart && a->dl > a->D0) return fail(TTX_ERR_INVALID, "ttx_debug_bs_prep: dl exceeds the drafts' D0");
  if (a->smart && (a->n_lib < 1 || a->dl + 1 > a->lib_ld)) return fail(TTX_ERR_INVALID, "ttx_debug_bs_prep: smart mode needs n_lib >= 1 and lib_ld >= dl + 1");
  HIP_TRY(hipSetDevice(s->m->device));
  BeamPrepArgs pa{};
  pa.cand_next = a->d_cand_next; pa.ld = a->ld; pa.len_next = a->d_len_next; pa.fin_next = a->d_fin_next; pa.logp_next = a->d_logp_next;
  pa.n_cand = a->n_cand; pa.beam = a->beam; pa.dl = a->dl; pa.N = a->N; pa.pad = a->pad;
  pa.smart = a->smart ? 1 : 0; pa.n_lib = a->n_lib; pa.lib_ld = a->lib_ld; pa.drafts_all = a->d_drafts_all; pa.D0 = a->D0; pa.lib = a->d_lib;
  pa.gen = a->d_gen; pa.front = a->d_front; pa.len = a->d_len; pa.active = a->d_active; pa.finished = a->d_finished; pa.logp = a->d_logp;
  pa.per_cand = a->d_per_cand; pa.drafts32 = a->d_drafts32;
  return dbg_launched(launch_bs_prep(st, a->max_cand, pa), st);
}

extern "C" int ttx_debug_bs_list(ttx_session* s, const ttx_debug_bs_list_args* a, int64_t* words, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !a || !words) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_bs_list");
  if (!a->d_active || !a->d_per_cand || !a->d_len || !a->d_act_idx || !a->d_slot_of || !a->d_prev_len || !a->d_summary)
    return fail(TTX_ERR_INVALID, "ttx_debug_bs_list: a required array is null");
  if (a->n_cand < 0 || a->N < 1 || a->N > BS_MAX_SLOTS || a->dl < 0) return fail(TTX_ERR_INVALID, "ttx_debug_bs_list: n_cand, dl >= 0 and N in [1, 64]");
  HIP_TRY(hipSetDevice(s->m->device));
  struct Image { BeamCounters cnt; DecState st; };
  Image* dev = nullptr;
  HIP_TRY(hipMalloc((void**)&dev, sizeof(Image)));
  Image h{};
  h.cnt.model_calls = words[0]; h.cnt.input_lines = words[1]; h.cnt.running_rows = words[2]; h.cnt.verified_positions = words[3];
  h.cnt.executed_positions = words[4]; h.cnt.kv_prefix_positions = words[5]; h.cnt.running_cands = words[6]; h.cnt.max_group = (int)words[7];
  std::memset(&h.st, 0xAA, sizeof(DecState));          // the kernel writes every word of the DecState
  hipError_t err = hipMemcpyAsync(dev, &h, sizeof(Image), hipMemcpyHostToDevice, st);
  int rc = TTX_OK;
  if (err == hipSuccess) {
    BeamListArgs la{};
    la.active = a->d_active; la.per_cand = a->d_per_cand; la.len = a->d_len; la.n_cand = a->n_cand; la.N = a->N; la.dl = a->dl;
    la.act_idx = a->d_act_idx; la.slot_of = a->d_slot_of; la.prev_len = a->d_prev_len; la.st = &dev->st; la.cnt = &dev->cnt;
    la.summary = a->d_summary;
    rc = launch_bs_list(st, la);
  }
  if (err == hipSuccess && rc == TTX_OK) err = hipMemcpyAsync(&h, dev, sizeof(Image), hipMemcpyDeviceToHost, st);
  const hipError_t esync = hipStreamSynchronize(st);
  (void)hipFree(dev);
  TTX_TRY(rc);
  HIP_TRY(err);
  HIP_TRY(esync);
  words[0] = h.cnt.model_calls; words[1] = h.cnt.input_lines; words[2] = h.cnt.running_rows; words[3] = h.cnt.verified_positions;
  words[4] = h.cnt.executed_positions; words[5] = h.cnt.kv_prefix_positions; words[6] = h.cnt.running_cands; words[7] = h.cnt.max_group;
  const DecState& d = h.st;
  words[8] = d.n_active; words[9] = d.r_rows; words[10] = d.m_rows; words[11] = d.stop; words[12] = d.width; words[13] = d.steps;
  words[14] = d.error; words[15] = d.n_copy; words[16] = d.accepted; words[17] = d.produced; words[18] = d.verified_positions;
  words[19] = d.kv_prefix_positions; words[20] = d.src_positions;
  return TTX_OK;
}

extern "C" int ttx_debug_bs_hits(ttx_session* s, const ttx_debug_bs_hits_args* a, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !a) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_bs_hits");
  if (!a->d_logits || !a->d_finished || !a->d_slot_of || !a->d_per_cand || !a->d_drafts32 || !a->d_hit)
    return fail(TTX_ERR_INVALID, "ttx_debug_bs_hits: a required array is null");
  TTX_TRY(dbg_beam_limits("ttx_debug_bs_hits", a->K, a->N, a->V, a->dl));
  TTX_TRY(dbg_vpl("ttx_debug_bs_hits", a->vpl, a->V));
  if (a->max_cand < 1 || a->n_cand < 0 || a->n_cand > a->max_cand) return fail(TTX_ERR_INVALID, "ttx_debug_bs_hits: n_cand must lie in [0, max_cand]");
  HIP_TRY(hipSetDevice(s->m->device));
  BeamHitsArgs ha{};
  ha.logits = a->d_logits; ha.V = a->V; ha.finished = a->d_finished; ha.slot_of = a->d_slot_of; ha.per_cand = a->d_per_cand;
  ha.drafts32 = a->d_drafts32; ha.n_cand = a->n_cand; ha.N = a->N; ha.dl = a->dl; ha.K = a->K; ha.nucleus = BS_NUCLEUS;
  ha.hit = a->d_hit; ha.dl_of = a->d_dl_of;
  return dbg_launched(launch_hits_leaves(st, a->max_cand, &ha, nullptr, a->vpl), st);
}

extern "C" int ttx_debug_bs_leaves(ttx_session* s, const ttx_debug_bs_leaves_args* a, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !a) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_bs_leaves");
  if (!a->d_logits || !a->d_finished || !a->d_slot_of || !a->d_per_cand || !a->d_drafts32 || !a->d_logp || !a->d_hit || !a->d_best_n ||
      !a->d_best_slot || !a->d_chosen || !a->d_leaf_score || !a->d_leaf_tok || !a->d_leaf_cnt)
    return fail(TTX_ERR_INVALID, "ttx_debug_bs_leaves: a required array is null");
  TTX_TRY(dbg_beam_limits("ttx_debug_bs_leaves", a->K, a->N, a->V, a->dl));
  TTX_TRY(dbg_vpl("ttx_debug_bs_leaves", a->vpl, a->V));
  if (a->max_cand < 1 || a->n_cand < 0 || a->n_cand > a->max_cand) return fail(TTX_ERR_INVALID, "ttx_debug_bs_leaves: n_cand must lie in [0, max_cand]");
  if (!a->d_grp_of != !a->d_cand_batch) return fail(TTX_ERR_INVALID, "ttx_debug_bs_leaves: grp_of and cand_batch come together");
  if (a->smart && !a->d_grp_of && (a->max_group < 1 || a->max_group > a->N))
    return fail(TTX_ERR_INVALID, "ttx_debug_bs_leaves: max_group must lie in [1, N]");
  HIP_TRY(hipSetDevice(s->m->device));
  BeamCounters* cnt = nullptr;
  HIP_TRY(hipMalloc((void**)&cnt, sizeof(BeamCounters)));
  BeamCounters hc{};
  hc.max_group = a->max_group;
  const hipError_t err = hipMemcpyAsync(cnt, &hc, sizeof(BeamCounters), hipMemcpyHostToDevice, st);
  int rc = TTX_OK;
  if (err == hipSuccess) {
    BeamLeaves2Args le{};
    le.logits = a->d_logits; le.V = a->V; le.finished = a->d_finished; le.slot_of = a->d_slot_of; le.per_cand = a->d_per_cand;
    le.drafts32 = a->d_drafts32; le.logp = a->d_logp; le.hit = a->d_hit; le.cnt = cnt;
    le.n_cand = a->n_cand; le.N = a->N; le.dl = a->dl; le.K = a->K; le.bos = a->bos; le.pad = a->pad; le.smart = a->smart ? 1 : 0;
    le.best_n = a->d_best_n; le.best_slot = a->d_best_slot; le.chosen = a->d_chosen;
    le.leaf_score = a->d_leaf_score; le.leaf_tok = a->d_leaf_tok; le.leaf_cnt = a->d_leaf_cnt;
    le.live = a->d_live; le.dl_of = a->d_dl_of; le.grp_of = a->d_grp_of; le.cand_batch = a->d_cand_batch;
    rc = launch_hits_leaves(st, a->max_cand, nullptr, &le, a->vpl);
  }
  const hipError_t esync = hipStreamSynchronize(st);
  (void)hipFree(cnt);
  TTX_TRY(rc);
  HIP_TRY(err);
  HIP_TRY(esync);
  return TTX_OK;
}

extern "C" int ttx_debug_beam_select(ttx_session* s, const ttx_debug_beam_select_args* a, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !a) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_beam_select");
  if (!a->d_leaf_score || !a->d_leaf_tok || !a->d_leaf_cnt || !a->d_cand || !a->d_len || !a->d_chosen || !a->d_chosen_slot ||
      !a->d_finished || !a->d_new_cand || !a->d_new_logp || !a->d_parent || !a->d_parent_draft || !a->d_mark || !a->d_summary)
    return fail(TTX_ERR_INVALID, "ttx_debug_beam_select: a required array is null");
  if (!a->d_new_len != !a->d_new_finished) return fail(TTX_ERR_INVALID, "ttx_debug_beam_select: new_len and new_finished come together");
  if (a->B < 1 || a->beam < 1 || a->beam > NUC_MAX_KEEP || a->K < 1 || a->K > NUC_MAX_KEEP || a->dl < 0)
    return fail(TTX_ERR_INVALID, "ttx_debug_beam_select: B >= 1, beam and K in [1, 32], dl >= 0");
  const size_t nseg = (size_t)a->beam * (a->dl + 1);
  if (nseg > 1023 || (size_t)a->K * (a->dl + 1) > 1023 || 2 * nseg * a->K * 4 > 150 * 1024)
    return fail(TTX_ERR_INVALID, "ttx_debug_beam_select: too many leaves per source for the selection kernel's LDS image");
  if (a->width < 1 || a->width > a->ld_in || a->width > a->ld_out) return fail(TTX_ERR_INVALID, "ttx_debug_beam_select: width must lie in [1, min(ld_in, ld_out)]");
  HIP_TRY(hipSetDevice(s->m->device));
  BeamSelectArgs<int> sa{a->d_leaf_score, a->d_leaf_tok, a->d_leaf_cnt, a->d_cand, a->width, a->ld_in, a->ld_out, a->d_len, a->d_chosen,
                         a->d_chosen_slot, a->d_finished, a->B, a->beam, a->dl, a->K, a->pad, a->eos, a->d_new_cand, a->d_new_logp,
                         a->d_parent, a->d_parent_draft, a->d_mark, a->d_summary, a->d_new_len, a->d_new_finished};
  return dbg_launched(launch_beam_select(s, st, sa), st);
}

// The operands of a k_beam_step / k_beam_step_masked debug launch, checked, as the kernels' argument block.
static int beam_step_debug_args(const char* who_c, ttx_session* s, const ttx_debug_beam_step_args* a, BeamStepArgs* out) {
  const std::string who(who_c);
  if (!s || !a) return fail(TTX_ERR_INVALID, "null argument to " + who);
  if (!a->d_logits || !a->d_slot_of || !a->d_finished || !a->d_score || !a->d_gen || !a->d_new_cand || !a->d_new_score || !a->d_parent ||
      !a->d_new_len || !a->d_new_finished || !a->d_parent_draft || !a->d_summary)
    return fail(TTX_ERR_INVALID, who + ": a required array is null");
  if (a->B < 1 || a->beam < 1 || a->K < 1 || a->V < 1 || a->V > 64 * NUC_VPL) return fail(TTX_ERR_INVALID, who + ": B, beam, K >= 1 and V in [1, 1024]");
  if ((size_t)a->K > (size_t)a->beam * a->V) return fail(TTX_ERR_INVALID, who + ": K exceeds the beam * V totals");
  if ((size_t)a->beam * a->V * 4 > 150 * 1024) return fail(TTX_ERR_INVALID, who + ": beam x vocabulary beyond the selection kernel's LDS image");
  if (a->width < 1 || a->width >= a->ld) return fail(TTX_ERR_INVALID, who + ": width must lie in [1, ld)");
  BeamStepArgs sa{};
  sa.logits = a->d_logits; sa.V = a->V; sa.slot_of = a->d_slot_of; sa.finished = a->d_finished; sa.score = a->d_score;
  sa.gen = a->d_gen; sa.ld = a->ld; sa.width = a->width; sa.B = a->B; sa.beam = a->beam; sa.K = a->K; sa.pad = a->pad; sa.eos = a->eos;
  sa.new_cand = a->d_new_cand; sa.new_score = a->d_new_score; sa.parent = a->d_parent; sa.new_len = a->d_new_len;
  sa.new_finished = a->d_new_finished; sa.parent_draft = a->d_parent_draft; sa.summary = a->d_summary;
  *out = sa;
  return TTX_OK;
}

extern "C" int ttx_debug_beam_step(ttx_session* s, const ttx_debug_beam_step_args* a, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  BeamStepArgs sa{};
  TTX_TRY(beam_step_debug_args("ttx_debug_beam_step", s, a, &sa));
  HIP_TRY(hipSetDevice(s->m->device));
  return dbg_launched(launch_beam_step(s, st, sa), st);
}

extern "C" int ttx_debug_beam_step_masked(ttx_session* s, const ttx_debug_beam_step_args* a, const ttx_debug_prefix* pfx, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const char* who = "ttx_debug_beam_step_masked";
  BeamStepArgs sa{};
  TTX_TRY(beam_step_debug_args(who, s, a, &sa));
  HIP_TRY(hipSetDevice(s->m->device));
  PrefixTab tab{};
  if (pfx) {
    TTX_TRY(dbg_prefix_tab(who, pfx, a->B, st, &tab));
    if (a->width > pfx->ld) {           // a position beyond the table is forced for no source
      std::vector<int32_t> len((size_t)a->B);
      HIP_TRY(hipMemcpy(len.data(), pfx->d_len, (size_t)a->B * 4, hipMemcpyDeviceToHost));
      for (int b = 0; b < a->B; ++b)
        if (len[b] >= a->width) return fail(TTX_ERR_INVALID, "ttx_debug_beam_step_masked: width inside a prefix but beyond the table's ld");
    }
  }
  return dbg_launched(launch_beam_step_masked(s, st, sa, tab), st);
}

extern "C" int ttx_debug_beam_step_masked_launches(ttx_session* s) {
  return s ? (int)std::min<long long>(s->beam_step_masked_launches, 0x7fffffff) : 0;
}

// The operands of a k_sbs_step / k_sbs_step_masked debug launch, checked, as the kernels' argument block.
static int sbs_debug_args(const char* who_c, ttx_session* s, const ttx_debug_sbs_step_args* a, SbsStepArgs* out) {
  const std::string who(who_c);
  if (!s || !a) return fail(TTX_ERR_INVALID, "null argument to " + who);
  if (!a->d_logits || !a->d_slot_of || !a->d_finished || !a->d_phi || !a->d_g || !a->d_gen || !a->d_new_cand || !a->d_new_phi || !a->d_new_g ||
      !a->d_parent || !a->d_new_len || !a->d_new_finished || !a->d_parent_draft || !a->d_summary)
    return fail(TTX_ERR_INVALID, who + ": a required array is null");
  if (!a->d_tr_parent != !a->d_tr_token || !a->d_tr_parent != !a->d_tr_phi || !a->d_tr_parent != !a->d_tr_g)
    return fail(TTX_ERR_INVALID, who + ": the four trace arrays come together");
  if (a->B < 1 || a->beam < 1 || a->beam > SBS_MAX_BEAM || a->K < 1 || a->K > SBS_MAX_BEAM || a->V < 1 || a->V > SBS_MAX_V)
    return fail(TTX_ERR_INVALID, who + ": B >= 1, beam and K in [1, 32] and V in [1, 1024]");
  if ((size_t)a->K > (size_t)a->beam * a->V) return fail(TTX_ERR_INVALID, who + ": K exceeds the beam * V children");
  if ((size_t)a->beam * a->V * 4 > 150 * 1024) return fail(TTX_ERR_INVALID, who + ": beam x vocabulary beyond the kernel's LDS image");
  if (a->width < 1 || a->width >= a->ld) return fail(TTX_ERR_INVALID, who + ": width must lie in [1, ld)");
  if (a->pos < 1) return fail(TTX_ERR_INVALID, who + ": pos starts at 1");
  if (!(a->inv_T > 0.0f) || !std::isfinite(a->inv_T)) return fail(TTX_ERR_INVALID, who + ": inv_T must be finite and > 0");
  SbsStepArgs sa{};
  sa.logits = a->d_logits; sa.V = a->V; sa.slot_of = a->d_slot_of; sa.finished = a->d_finished; sa.phi = a->d_phi; sa.g = a->d_g;
  sa.gen = a->d_gen; sa.ld = a->ld; sa.width = a->width; sa.B = a->B; sa.beam = a->beam; sa.K = a->K; sa.pad = a->pad; sa.eos = a->eos;
  sa.row_keys = a->d_key; sa.seed = a->seed; sa.pos = a->pos; sa.inv_T = a->inv_T;
  sa.new_cand = a->d_new_cand; sa.new_phi = a->d_new_phi; sa.new_g = a->d_new_g; sa.parent = a->d_parent; sa.new_len = a->d_new_len;
  sa.new_finished = a->d_new_finished; sa.parent_draft = a->d_parent_draft; sa.summary = a->d_summary;
  sa.tr_parent = a->d_tr_parent; sa.tr_token = a->d_tr_token; sa.tr_phi = a->d_tr_phi; sa.tr_g = a->d_tr_g;
  *out = sa;
  return TTX_OK;
}

extern "C" int ttx_debug_sbs_step(ttx_session* s, const ttx_debug_sbs_step_args* a, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SbsStepArgs sa{};
  TTX_TRY(sbs_debug_args("ttx_debug_sbs_step", s, a, &sa));
  HIP_TRY(hipSetDevice(s->m->device));
  return dbg_launched(launch_sbs_step(s, st, sa), st);
}

extern "C" int ttx_debug_sbs_step_ex(ttx_session* s, const ttx_debug_sbs_step_args* a, int top_k, float top_p, const ttx_debug_prefix* pfx,
                                     int waves, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const char* who = "ttx_debug_sbs_step_ex";
  SbsStepArgs sa{};
  TTX_TRY(sbs_debug_args(who, s, a, &sa));
  if (top_k < 0 || top_k > SAMPLE_MAX_KEEP) return fail(TTX_ERR_INVALID, "ttx_debug_sbs_step_ex: top_k must be 0 or in [1, 32]");
  if (!(top_p > 0.0f) || !(top_p <= 1.0f)) return fail(TTX_ERR_INVALID, "ttx_debug_sbs_step_ex: top_p must be in (0, 1]");
  if (waves != 0 && waves != 4 && waves != 8 && waves != SBS_MASKED_MAX_WAVES)
    return fail(TTX_ERR_INVALID, "ttx_debug_sbs_step_ex: waves must be 0 (the production choice), 4, 8 or 16");
  HIP_TRY(hipSetDevice(s->m->device));
  sa.top_p = top_p;
  sa.top_k = (top_k == 0 && top_p < 1.0f) ? SAMPLE_MAX_KEEP : top_k;
  if (pfx) {
    TTX_TRY(dbg_prefix_tab(who, pfx, a->B, st, &sa.pfx));
    if (a->pos > pfx->ld) {             // a position beyond the table is forced for no source
      std::vector<int32_t> len((size_t)a->B);
      HIP_TRY(hipMemcpy(len.data(), pfx->d_len, (size_t)a->B * 4, hipMemcpyDeviceToHost));
      for (int b = 0; b < a->B; ++b)
        if (len[b] >= a->pos) return fail(TTX_ERR_INVALID, "ttx_debug_sbs_step_ex: pos inside a prefix but beyond the table's ld");
    }
  }
  return dbg_launched(launch_sbs_step_masked(s, st, sa, waves), st);
}

extern "C" int ttx_debug_tree_cache(ttx_session* s, const ttx_debug_tree_cache_args* a, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !a) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_tree_cache");
  if (!a->d_len || !a->d_parent || !a->d_parent_draft || !a->d_prev_len || !a->d_active || !a->d_k_old || !a->d_v_old || !a->d_k_new ||
      !a->d_v_new || !a->d_qkv_prev || !a->d_prev_slot_of)
    return fail(TTX_ERR_INVALID, "ttx_debug_tree_cache: a required array is null");
  if (!a->d_slot_parent != !a->d_slot_self) return fail(TTX_ERR_INVALID, "ttx_debug_tree_cache: slot_parent and slot_self come together");
  if (a->d_slot_self && (a->d_k_old != a->d_k_new || a->d_v_old != a->d_v_new))
    return fail(TTX_ERR_INVALID, "ttx_debug_tree_cache: with slot maps there is one cache buffer");
  if (a->max_cand < 1 || a->layers < 1 || a->prev_N < 1 || a->prev_N > BS_MAX_SLOTS || a->prev_D < 0 || a->d < 4 || (a->d & 3))
    return fail(TTX_ERR_INVALID, "ttx_debug_tree_cache: max_cand, layers >= 1, prev_N in [1, 64], prev_D >= 0, d a positive multiple of 4");
  if ((a->cache_layer_stride & 3) || (a->cache_seq_stride & 3) || (a->qkv_layer_stride & 3) || a->cache_seq_stride < a->d ||
      a->cache_layer_stride < a->cache_seq_stride || a->qkv_layer_stride < 3 * a->d)
    return fail(TTX_ERR_INVALID, "ttx_debug_tree_cache: strides must be multiples of 4 floats that cover their rows");
  if (!dbg_aligned16(a->d_k_old) || !dbg_aligned16(a->d_v_old) || !dbg_aligned16(a->d_k_new) || !dbg_aligned16(a->d_v_new) ||
      !dbg_aligned16(a->d_qkv_prev))
    return fail(TTX_ERR_INVALID, "ttx_debug_tree_cache: float operands must be 16-byte aligned");
  HIP_TRY(hipSetDevice(s->m->device));
  TreeCacheArgs ca{};
  ca.len = a->d_len; ca.parent = a->d_parent; ca.parent_draft = a->d_parent_draft; ca.prev_len = a->d_prev_len; ca.active = a->d_active;
  ca.k_old = a->d_k_old; ca.v_old = a->d_v_old; ca.k_new = a->d_k_new; ca.v_new = a->d_v_new;
  ca.cache_layer_stride = a->cache_layer_stride; ca.cache_seq_stride = a->cache_seq_stride;
  ca.qkv_prev = a->d_qkv_prev; ca.qkv_layer_stride = a->qkv_layer_stride; ca.prev_slot_of = a->d_prev_slot_of;
  ca.prev_N = a->prev_N; ca.prev_D = a->prev_D; ca.d = a->d; ca.slot_parent = a->d_slot_parent; ca.slot_self = a->d_slot_self;
  return dbg_launched(launch_tree_cache(st, a->max_cand, a->layers, ca), st);
}

// ---- the pool's bookkeeping kernels, one launch per call through launch_bsp_* ---------------------------------------------------
extern "C" int ttx_debug_bsp(ttx_session* s, int op, const ttx_debug_bsp_args* a, int64_t* words, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const std::string w = "ttx_debug_bsp";
  enum { OP_INIT, OP_ADMIT, OP_FILL, OP_PREP, OP_SELECT, OP_BATCHES, OP_RETIRE, OP_PUBLISH, OP_COUNT };
  if (!s || !a || !words) return fail(TTX_ERR_INVALID, "null argument to " + w);
  if (op < 0 || op >= OP_COUNT) return fail(TTX_ERR_INVALID, w + ": op is 0 (init) .. 7 (publish)");
  if (!a->d_row_of || !a->d_slot_batch || !a->d_src_acc || !a->d_src_state || !a->d_tok || (!a->smart && !a->d_drafts_all) || !a->d_bat_id ||
      !a->d_bat_iter || !a->d_bat_dl || !a->d_bat_grp || !a->d_bat_live || !a->d_bat_nfin || !a->d_bat_longest_fin || !a->d_bat_longest_cur ||
      !a->d_bat_state || !a->d_bat_given || !a->d_cand_next || !a->d_len_next || !a->d_fin_next || !a->d_logp_next || !a->d_parent ||
      !a->d_parent_draft || !a->d_gen || !a->d_front || !a->d_len || !a->d_active || !a->d_finished || !a->d_live || !a->d_logp ||
      !a->d_per_cand || !a->d_drafts32 || !a->d_cand_dl || !a->d_cand_batch || !a->d_cache_slot || !a->d_cache_slot_parent ||
      !a->d_chosen_slot || !a->d_chosen || !a->d_leaf_score || !a->d_leaf_tok || !a->d_leaf_cnt || !a->d_dev_summary)
    return fail(TTX_ERR_INVALID, w + ": an array of the pool's argument block is null");
  if (!a->d_out || !a->d_trace_len || !a->d_summary || !a->d_len_all || !a->d_batch_all || !a->d_given_all)
    return fail(TTX_ERR_INVALID, w + ": a caller-side array is null");
  if (op == OP_INIT && (!a->d_src_of || !a->d_cand_src_len)) return fail(TTX_ERR_INVALID, w + ": init needs src_of and cand_src_len");
  if (op == OP_ADMIT && (!a->d_new_slot || !a->d_cand_src_len)) return fail(TTX_ERR_INVALID, w + ": admit needs new_slot and cand_src_len");
  if (op == OP_FILL && (!a->d_new_slot || !a->d_tok_new || !a->d_valid_new || !a->d_src_valid || !a->d_memkv || !a->d_memkv_new))
    return fail(TTX_ERR_INVALID, w + ": fill needs new_slot, tok_new, valid_new, src_valid, memkv and memkv_new");
  if (a->C < 1 || a->K < 1 || a->N < 1 || a->D0 < 0 || a->Ls_cap < 1 || a->max_len < 1 || a->ld < 1 || a->T_cap < 1 || a->max_steps < 0)
    return fail(TTX_ERR_INVALID, w + ": C, K, N, Ls_cap, max_len, ld and T_cap must be positive, D0 and max_steps >= 0");
  if (a->C > 1024 || a->K > NUC_MAX_KEEP || a->N > BS_MAX_SLOTS) return fail(TTX_ERR_INVALID, w + ": C <= 1024, K <= 32 and N <= 64");
  if ((size_t)a->K * (a->D0 + 1) > 1023 || bsp_select_lds(a->K, a->D0) > 150 * 1024)
    return fail(TTX_ERR_INVALID, w + ": too many leaves per source for the selection kernel's LDS image");
  if (a->ld < a->max_len + a->D0 + 2) return fail(TTX_ERR_INVALID, w + ": ld must cover max_len + D0 + 2 columns");
  if (op == OP_ADMIT || op == OP_FILL) {
    if (a->R < 1 || a->first_row < 0) return fail(TTX_ERR_INVALID, w + ": R must be positive and first_row >= 0");
    if (a->R > a->C) return fail(TTX_ERR_INVALID, w + ": more new sources than the pool has slots");
  }
  if (op == OP_FILL) {
    if (a->Ls_new < 1 || a->Ls_new > a->Ls_cap) return fail(TTX_ERR_INVALID, w + ": Ls_new must lie in [1, Ls_cap]");
    if (a->kv_row < 4 || (a->kv_row & 3)) return fail(TTX_ERR_INVALID, w + ": kv_row must be a positive multiple of 4");
    if (!dbg_aligned16(a->d_memkv) || !dbg_aligned16(a->d_memkv_new)) return fail(TTX_ERR_INVALID, w + ": memkv operands must be 16-byte aligned");
  }
  HIP_TRY(hipSetDevice(s->m->device));
  if (!s->bp_host && hipHostMalloc((void**)&s->bp_host, sizeof(BeamPoolHost), hipHostMallocMapped) != hipSuccess)
    return fail(TTX_ERR_NOMEM, "hipHostMalloc failed");
  BeamPoolHost* dev_host = nullptr;
  HIP_TRY(hipHostGetDevicePointer((void**)&dev_host, (void*)s->bp_host, 0));
  HIP_TRY(hipStreamSynchronize(st));                    // nothing in flight reads the pinned words while the image goes in
  s->bp_host->steps_done = (int)words[8]; s->bp_host->n_live = (int)words[9]; s->bp_host->n_running = (int)words[10];
  s->bp_host->error = (int)words[11];
  struct Image { BeamCounters cnt; BeamPoolIo io; };
  Image* dev = nullptr;
  HIP_TRY(hipMalloc((void**)&dev, sizeof(Image)));
  Image h{};
  h.cnt.model_calls = words[0]; h.cnt.input_lines = words[1]; h.cnt.running_rows = words[2]; h.cnt.verified_positions = words[3];
  h.cnt.executed_positions = words[4]; h.cnt.kv_prefix_positions = words[5]; h.cnt.running_cands = words[6]; h.cnt.max_group = (int)words[7];
  h.io.out = a->d_out; h.io.trace_len = a->d_trace_len; h.io.summary = a->d_summary; h.io.len_all = a->d_len_all;
  h.io.batch_all = a->d_batch_all; h.io.given_all = a->d_given_all; h.io.T_cap = a->T_cap;
  hipError_t err = hipMemcpyAsync(dev, &h, sizeof(Image), hipMemcpyHostToDevice, st);
  int rc = TTX_OK;
  if (err == hipSuccess) {
    BeamPoolArgs p{};
    p.C = a->C; p.K = a->K; p.N = a->N; p.D0 = a->D0; p.Ls_cap = a->Ls_cap; p.max_len = a->max_len; p.ld = a->ld;
    p.smart = a->smart ? 1 : 0; p.lib_ld = a->lib_ld; p.pad = a->pad; p.bos = a->bos; p.eos = a->eos; p.repl = a->repl; p.max_steps = a->max_steps;
    p.row_of = a->d_row_of; p.slot_batch = a->d_slot_batch; p.src_acc = a->d_src_acc; p.src_state = a->d_src_state;
    p.tok = a->d_tok; p.drafts_all = a->d_drafts_all;
    p.bat_id = a->d_bat_id; p.bat_iter = a->d_bat_iter; p.bat_dl = a->d_bat_dl; p.bat_grp = a->d_bat_grp; p.bat_live = a->d_bat_live;
    p.bat_nfin = a->d_bat_nfin; p.bat_longest_fin = a->d_bat_longest_fin; p.bat_longest_cur = a->d_bat_longest_cur;
    p.bat_state = a->d_bat_state; p.bat_given = a->d_bat_given;
    p.cand_next = a->d_cand_next; p.len_next = a->d_len_next; p.fin_next = a->d_fin_next; p.logp_next = a->d_logp_next;
    p.parent = a->d_parent; p.parent_draft = a->d_parent_draft;
    p.gen = a->d_gen; p.front = a->d_front; p.len = a->d_len; p.active = a->d_active; p.finished = a->d_finished; p.live = a->d_live;
    p.logp = a->d_logp; p.per_cand = a->d_per_cand; p.drafts32 = a->d_drafts32; p.cand_dl = a->d_cand_dl; p.cand_batch = a->d_cand_batch;
    p.cache_slot = a->d_cache_slot; p.cache_slot_parent = a->d_cache_slot_parent;
    p.chosen_slot = a->d_chosen_slot; p.chosen = a->d_chosen; p.leaf_score = a->d_leaf_score; p.leaf_tok = a->d_leaf_tok; p.leaf_cnt = a->d_leaf_cnt;
    p.cnt = &dev->cnt; p.io = &dev->io; p.host = dev_host; p.dev_summary = a->d_dev_summary;
    switch (op) {
      case OP_INIT: rc = launch_bsp_init(st, p, a->d_src_of, a->d_cand_src_len); break;
      case OP_ADMIT: rc = launch_bsp_admit(st, p, a->d_new_slot, a->d_cand_src_len, a->R, a->first_row); break;
      case OP_FILL:
        rc = launch_bsp_fill(st, bsp_fill_args(p, a->d_new_slot, a->R, a->first_row, a->Ls_new, a->d_tok_new, a->d_src_valid, a->d_valid_new,
                                               a->d_drafts_new, a->d_memkv, a->d_memkv_new, a->kv_row));
        break;
      case OP_PREP: rc = launch_bsp_prep(st, p); break;
      case OP_SELECT: rc = launch_bsp_select(s, st, p); break;
      case OP_BATCHES: rc = launch_bsp_batches(st, p); break;
      case OP_RETIRE: rc = launch_bsp_retire(st, p); break;
      default: rc = launch_bsp_publish(st, p); break;
    }
  }
  if (err == hipSuccess && rc == TTX_OK) err = hipMemcpyAsync(&h, dev, sizeof(Image), hipMemcpyDeviceToHost, st);
  const hipError_t esync = hipStreamSynchronize(st);
  (void)hipFree(dev);
  TTX_TRY(rc);
  HIP_TRY(err);
  HIP_TRY(esync);
  words[0] = h.cnt.model_calls; words[1] = h.cnt.input_lines; words[2] = h.cnt.running_rows; words[3] = h.cnt.verified_positions;
  words[4] = h.cnt.executed_positions; words[5] = h.cnt.kv_prefix_positions; words[6] = h.cnt.running_cands; words[7] = h.cnt.max_group;
  words[8] = s->bp_host->steps_done; words[9] = s->bp_host->n_live; words[10] = s->bp_host->n_running; words[11] = s->bp_host->error;
  return TTX_OK;
}

// The stochastic beam pool's step kernels, one launch (tests/test_gpu_sbs_pool_kernel.py).
extern "C" int ttx_debug_sbs_step_pool(ttx_session* s, const ttx_debug_sbs_step_pool_args* a, int masked, int top_k, float top_p,
                                       const ttx_debug_prefix* pfx, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const std::string w = "ttx_debug_sbs_step_pool";
  if (!s || !a) return fail(TTX_ERR_INVALID, "null argument to " + w);
  if (!a->d_logits || !a->d_slot_of || !a->d_finished || !a->d_phi || !a->d_g || !a->d_gen || !a->d_row_of || !a->d_level || !a->d_nlive ||
      !a->d_key || !a->d_new_cand || !a->d_new_phi || !a->d_new_g || !a->d_parent || !a->d_new_len || !a->d_new_finished || !a->d_parent_draft ||
      !a->d_nfin)
    return fail(TTX_ERR_INVALID, w + ": a required array is null");
  if (a->C < 1 || a->C > 1024 || a->K < 1 || a->K > SBS_MAX_BEAM || a->V < 1 || a->V > SBS_MAX_V)
    return fail(TTX_ERR_INVALID, w + ": C in [1, 1024], K in [1, 32] and V in [1, 1024]");
  if (a->K > a->V) return fail(TTX_ERR_INVALID, w + ": K exceeds the V children of a fresh slot");
  if ((size_t)a->K * a->V * 4 > 150 * 1024) return fail(TTX_ERR_INVALID, w + ": K x vocabulary beyond the kernel's LDS image");
  if (a->ld < 2) return fail(TTX_ERR_INVALID, w + ": ld must be at least 2");
  if (!(a->inv_T > 0.0f) || !std::isfinite(a->inv_T)) return fail(TTX_ERR_INVALID, w + ": inv_T must be finite and > 0");
  if (!masked && (top_k != 0 || top_p != 1.0f || pfx)) return fail(TTX_ERR_INVALID, w + ": a filter or a prefix table needs the masked kernel");
  if (top_k < 0 || top_k > SAMPLE_MAX_KEEP) return fail(TTX_ERR_INVALID, w + ": top_k must be 0 or in [1, 32]");
  if (!(top_p > 0.0f) || !(top_p <= 1.0f)) return fail(TTX_ERR_INVALID, w + ": top_p must be in (0, 1]");
  HIP_TRY(hipSetDevice(s->m->device));
  HIP_TRY(hipStreamSynchronize(st));
  std::vector<int32_t> slot((size_t)a->C * 3);
  HIP_TRY(hipMemcpy(slot.data(), a->d_row_of, (size_t)a->C * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(slot.data() + a->C, a->d_level, (size_t)a->C * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(slot.data() + 2 * a->C, a->d_nlive, (size_t)a->C * 4, hipMemcpyDeviceToHost));
  for (int b = 0; b < a->C; ++b) {
    if (slot[b] < 0) continue;
    if (slot[a->C + b] < 1 || slot[a->C + b] >= a->ld) return fail(TTX_ERR_INVALID, w + ": a live slot's level must lie in [1, ld)");
    if (slot[2 * a->C + b] < 1 || slot[2 * a->C + b] > a->K) return fail(TTX_ERR_INVALID, w + ": a live slot's parent count must lie in [1, K]");
  }
  SbsPoolStepArgs sa{};
  sa.logits = a->d_logits; sa.V = a->V; sa.slot_of = a->d_slot_of; sa.finished = a->d_finished; sa.phi = a->d_phi; sa.g = a->d_g;
  sa.gen = a->d_gen; sa.ld = a->ld; sa.C = a->C; sa.K = a->K; sa.pad = a->pad; sa.eos = a->eos;
  sa.row_of = a->d_row_of; sa.level = a->d_level; sa.nlive = a->d_nlive; sa.key = a->d_key; sa.seed = a->seed; sa.inv_T = a->inv_T;
  sa.new_cand = a->d_new_cand; sa.new_phi = a->d_new_phi; sa.new_g = a->d_new_g; sa.parent = a->d_parent; sa.new_len = a->d_new_len;
  sa.new_finished = a->d_new_finished; sa.parent_draft = a->d_parent_draft; sa.nfin = a->d_nfin;
  if (!masked) return dbg_launched(launch_sbs_step_pool(s, st, sa), st);
  sa.top_p = top_p;
  sa.top_k = (top_k == 0 && top_p < 1.0f) ? SAMPLE_MAX_KEEP : top_k;
  if (pfx) TTX_TRY(dbg_prefix_tab(w.c_str(), pfx, a->C, st, &sa.pfx));
  return dbg_launched(launch_sbs_step_pool_masked(s, st, sa), st);
}

// The stochastic beam pool's bookkeeping kernels, one launch per call (ttx_debug_bsp's conventions).
extern "C" int ttx_debug_sbs_pool(ttx_session* s, int op, const ttx_debug_sbs_pool_args* a, int64_t* words, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const std::string w = "ttx_debug_sbs_pool";
  enum { OP_INIT, OP_ADMIT, OP_FILL, OP_RETIRE, OP_PUBLISH, OP_COUNT };
  if (!s || !a || !words) return fail(TTX_ERR_INVALID, "null argument to " + w);
  if (op < 0 || op >= OP_COUNT) return fail(TTX_ERR_INVALID, w + ": op is 0 (init) .. 4 (publish)");
  if (!a->d_row_of || !a->d_level || !a->d_nlive || !a->d_nfin || !a->d_key || !a->d_pfx_len || !a->d_pfx_src || !a->d_run_acc || !a->d_cand_next ||
      !a->d_len_next || !a->d_fin_next || !a->d_phi_next || !a->d_parent || !a->d_parent_draft || !a->d_cand_src_len || !a->d_g_in ||
      !a->d_g_out || !a->d_len_all || !a->d_out || !a->d_out_logp || !a->d_out_gumbel || !a->d_dev_summary)
    return fail(TTX_ERR_INVALID, w + ": an array of the pool's argument block is null");
  if (op == OP_INIT && !a->d_src_of) return fail(TTX_ERR_INVALID, w + ": init needs src_of");
  if ((op == OP_ADMIT || op == OP_FILL) && !a->d_new_slot) return fail(TTX_ERR_INVALID, w + ": admit and fill need new_slot");
  if (op == OP_FILL && (!a->d_valid_new || !a->d_src_valid || !a->d_memkv || !a->d_memkv_new))
    return fail(TTX_ERR_INVALID, w + ": fill needs valid_new, src_valid, memkv and memkv_new");
  if (a->C < 1 || a->C > 1024 || a->K < 1 || a->K > SBS_MAX_BEAM || a->Ls_cap < 1 || a->max_len < 2 || a->ld < a->max_len)
    return fail(TTX_ERR_INVALID, w + ": C in [1, 1024], K in [1, 32], Ls_cap >= 1, max_len >= 2 and ld >= max_len");
  if (op == OP_ADMIT || op == OP_FILL) {
    if (a->R < 1 || a->first_row < 0 || a->R > a->C) return fail(TTX_ERR_INVALID, w + ": R must lie in [1, C] and first_row >= 0");
  }
  if (op == OP_FILL) {
    if (a->Ls_new < 1 || a->Ls_new > a->Ls_cap) return fail(TTX_ERR_INVALID, w + ": Ls_new must lie in [1, Ls_cap]");
    if (a->kv_row < 4 || (a->kv_row & 3)) return fail(TTX_ERR_INVALID, w + ": kv_row must be a positive multiple of 4");
    if (!dbg_aligned16(a->d_memkv) || !dbg_aligned16(a->d_memkv_new)) return fail(TTX_ERR_INVALID, w + ": memkv operands must be 16-byte aligned");
  }
  HIP_TRY(hipSetDevice(s->m->device));
  if (!s->bp_host && hipHostMalloc((void**)&s->bp_host, sizeof(BeamPoolHost), hipHostMallocMapped) != hipSuccess)
    return fail(TTX_ERR_NOMEM, "hipHostMalloc failed");
  BeamPoolHost* dev_host = nullptr;
  HIP_TRY(hipHostGetDevicePointer((void**)&dev_host, (void*)s->bp_host, 0));
  HIP_TRY(hipStreamSynchronize(st));                    // nothing in flight reads the pinned words while the image goes in
  s->bp_host->steps_done = (int)words[8]; s->bp_host->n_live = (int)words[9]; s->bp_host->n_running = (int)words[10];
  s->bp_host->error = (int)words[11];
  struct Image { BeamCounters cnt; SbsPoolIo io; };
  Image* dev = nullptr;
  HIP_TRY(hipMalloc((void**)&dev, sizeof(Image)));
  Image h{};
  h.cnt.model_calls = words[0]; h.cnt.input_lines = words[1]; h.cnt.running_rows = words[2]; h.cnt.verified_positions = words[3];
  h.cnt.executed_positions = words[4]; h.cnt.kv_prefix_positions = words[5]; h.cnt.running_cands = words[6]; h.cnt.max_group = (int)words[7];
  h.io = SbsPoolIo{a->d_out, a->d_out_logp, a->d_out_gumbel, a->d_src_running};
  hipError_t err = hipMemcpyAsync(dev, &h, sizeof(Image), hipMemcpyHostToDevice, st);
  int rc = TTX_OK;
  if (err == hipSuccess) {
    SbsPoolFillArgs f{};
    SbsPoolArgs& p = f.a;
    p.C = a->C; p.K = a->K; p.max_len = a->max_len; p.ld = a->ld; p.Ls_cap = a->Ls_cap; p.pad = a->pad; p.bos = a->bos;
    p.row_of = a->d_row_of; p.level = a->d_level; p.nlive = a->d_nlive; p.nfin = a->d_nfin; p.key = a->d_key; p.pfx_len = a->d_pfx_len;
    p.pfx_src = a->d_pfx_src; p.run_acc = a->d_run_acc;
    p.cand_next = a->d_cand_next; p.len_next = a->d_len_next; p.fin_next = a->d_fin_next; p.phi_next = a->d_phi_next; p.parent = a->d_parent;
    p.parent_draft = a->d_parent_draft; p.cand_src_len = a->d_cand_src_len; p.g_in = a->d_g_in; p.g_out = a->d_g_out;
    p.len_all = a->d_len_all; p.row_keys = a->d_row_keys; p.pfx_len_src = a->d_pfx_len_src;
    p.io = &dev->io;
    p.cnt = &dev->cnt; p.host = dev_host; p.dev_summary = a->d_dev_summary;
    f.new_slot = a->d_new_slot; f.R = a->R; f.first_row = a->first_row; f.Ls_new = a->Ls_new;
    f.src_valid = a->d_src_valid; f.valid_new = a->d_valid_new; f.memkv = a->d_memkv; f.memkv_new = a->d_memkv_new; f.kv_row = a->kv_row;
    switch (op) {
      case OP_INIT: rc = launch_sbsp_init(st, p, a->d_g_in, a->d_g_out, a->d_src_of); break;
      case OP_ADMIT: rc = launch_sbsp_admit(st, p, a->d_new_slot, a->R, a->first_row); break;
      case OP_FILL: rc = launch_sbsp_fill(st, f); break;
      case OP_RETIRE: rc = launch_sbsp_retire(st, p); break;
      default: rc = launch_sbsp_publish(st, p); break;
    }
  }
  if (err == hipSuccess && rc == TTX_OK) err = hipMemcpyAsync(&h, dev, sizeof(Image), hipMemcpyDeviceToHost, st);
  const hipError_t esync = hipStreamSynchronize(st);
  (void)hipFree(dev);
  TTX_TRY(rc);
  HIP_TRY(err);
  HIP_TRY(esync);
  words[0] = h.cnt.model_calls; words[1] = h.cnt.input_lines; words[2] = h.cnt.running_rows; words[3] = h.cnt.verified_positions;
  words[4] = h.cnt.executed_positions; words[5] = h.cnt.kv_prefix_positions; words[6] = h.cnt.running_cands; words[7] = h.cnt.max_group;
  words[8] = s->bp_host->steps_done; words[9] = s->bp_host->n_live; words[10] = s->bp_host->n_running; words[11] = s->bp_host->error;
  return TTX_OK;
}

static int kvcopy_debug(const char* who, ttx_session* s, const int32_t* d_rec, int n_copy, const float* d_qkv, int64_t qkv_layer_stride,
                        float* d_kcache, float* d_vcache, int64_t cache_layer_stride, int64_t cache_seq_stride, int N, int D, int d, int B,
                        int Ld, const int32_t* d_pos2, const float* d_qkv_probe, int64_t probe_layer_stride, hipStream_t st,
                        const int32_t* d_row_base = nullptr, const int32_t* d_draft_mask = nullptr) {
  const std::string w(who);
  if ((d_row_base || d_draft_mask) && !d_pos2) return fail(TTX_ERR_INVALID, w + ": row_base and draft_mask need pos2");
  if (!s || !d_rec || !d_qkv || !d_kcache || !d_vcache) return fail(TTX_ERR_INVALID, "null argument to " + w);
  if (!dbg_model_d(d)) return fail(TTX_ERR_INVALID, w + ": d must be 64, 128, 256, 512 or 1024");
  if (B < 1 || Ld < 1 || N < 1 || D < 0) return fail(TTX_ERR_INVALID, w + ": B, Ld and N must be positive, D >= 0");
  if (n_copy < 0 || n_copy > B) return fail(TTX_ERR_INVALID, w + ": n_copy must lie in [0, B]");
  if (!dbg_aligned16(d_qkv) || !dbg_aligned16(d_kcache) || !dbg_aligned16(d_vcache))
    return fail(TTX_ERR_INVALID, w + ": float operands must be 16-byte aligned");
  const int RPS = step_rps(N, D);
  if ((qkv_layer_stride & 3) || qkv_layer_stride < (int64_t)B * RPS * 3 * d)
    return fail(TTX_ERR_INVALID, w + ": qkv_layer_stride must be a multiple of 4 covering B * (1 + N*D) rows of 3d");
  if ((cache_seq_stride & 3) || cache_seq_stride < d || (cache_layer_stride & 3) || cache_layer_stride < (int64_t)B * cache_seq_stride)
    return fail(TTX_ERR_INVALID, w + ": the cache strides must be multiples of 4, a row's covering d and a layer's B rows");
  if ((d_pos2 != nullptr) != (d_qkv_probe != nullptr)) return fail(TTX_ERR_INVALID, w + ": pos2 and qkv_probe come together");
  if (d_pos2 && (!dbg_aligned16(d_qkv_probe) || (probe_layer_stride & 3) || probe_layer_stride < (int64_t)B * 3 * d))
    return fail(TTX_ERR_INVALID, w + ": qkv_probe must be 16-byte aligned and its layer stride a multiple of 4 covering B rows of 3d");
  HIP_TRY(hipSetDevice(s->m->device));
  if (n_copy > 0) {
    std::vector<CopyRec> rec((size_t)n_copy);
    std::vector<int> pos((size_t)n_copy, 0);
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(rec.data(), d_rec, (size_t)n_copy * sizeof(CopyRec), hipMemcpyDeviceToHost));
    if (d_pos2) HIP_TRY(hipMemcpy(pos.data(), d_pos2, (size_t)n_copy * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < n_copy; ++i) {
      const CopyRec& r = rec[i];
      if (r.b < 0 || r.b >= B || r.best < 0 || r.best >= N || r.nacc < 0 || r.nacc > D || r.front_old < 0 ||
          ((int64_t)r.front_old + r.nacc + 1) * d > cache_seq_stride)
        return fail(TTX_ERR_INVALID, w + ": a record is outside the operands (b, best, nacc or front_old + nacc + 1 positions)");
      if (d_pos2 && (pos[i] < -1 || pos[i] >= B || (pos[i] < 0 && r.nacc != 0)))
        return fail(TTX_ERR_INVALID, w + ": pos2 must lie in [-1, B), and a slot without a draft pass (-1) accepts nothing");
    }
    if (d_row_base || d_draft_mask) {
      int n_pos = 0, total = 0;
      for (int i = 0; i < n_copy; ++i) n_pos = std::max(n_pos, pos[i] + 1);
      std::vector<int32_t> mask;
      TTX_TRY(dbg_check_select(w, d_row_base, d_draft_mask, n_pos, N, D, st, &mask, &total));
      for (int i = 0; i < n_copy; ++i)
        if (pos[i] >= 0 && rec[i].nacc > 0 && !(((unsigned)mask[pos[i]] >> rec[i].best) & 1u))
          return fail(TTX_ERR_INVALID, w + ": the best draft of a slot that accepted tokens must be a present one");
    }
  }
  DecState* dst = nullptr;
  HIP_TRY(hipMalloc((void**)&dst, sizeof(DecState)));
  DecState* hs = reinterpret_cast<DecState*>(s->host_state);
  *hs = DecState{};
  hs->n_copy = n_copy;
  hipError_t err = hipMemcpyAsync(dst, hs, sizeof(DecState), hipMemcpyHostToDevice, st);
  if (err == hipSuccess) {
    KvCopyArgs kc{};
    kc.st = dst; kc.rec = reinterpret_cast<const CopyRec*>(d_rec); kc.qkv = d_qkv; kc.qkv_layer_stride = (long long)qkv_layer_stride;
    kc.kcache = d_kcache; kc.vcache = d_vcache; kc.cache_layer_stride = (long long)cache_layer_stride;
    kc.cache_seq_stride = (long long)cache_seq_stride; kc.N = N; kc.D = D; kc.d = d;
    kc.pos2 = d_pos2; kc.qkv_probe = d_qkv_probe; kc.probe_layer_stride = (long long)probe_layer_stride;
    kc.row_base = d_row_base; kc.draft_mask = d_draft_mask;
    hipLaunchKernelGGL(k_kvcopy, dim3(B, Ld), dim3(256), 0, st, kc);
    err = hipGetLastError();
  }
  const hipError_t esync = hipStreamSynchronize(st);
  (void)hipFree(dst);
  HIP_TRY(err);
  HIP_TRY(esync);
  return TTX_OK;
}

extern "C" int ttx_debug_kvcopy(ttx_session* s, const int32_t* d_rec, int n_copy, const float* d_qkv, int64_t qkv_layer_stride,
                                float* d_kcache, float* d_vcache, int64_t cache_layer_stride, int64_t cache_seq_stride, int N, int D,
                                int d, int B, int Ld, void* stream) {
  return kvcopy_debug("ttx_debug_kvcopy", s, d_rec, n_copy, d_qkv, qkv_layer_stride, d_kcache, d_vcache, cache_layer_stride,
                      cache_seq_stride, N, D, d, B, Ld, nullptr, nullptr, 0, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int ttx_debug_kvcopy_split(ttx_session* s, const int32_t* d_rec, int n_copy, const float* d_qkv, int64_t qkv_layer_stride,
                                      float* d_kcache, float* d_vcache, int64_t cache_layer_stride, int64_t cache_seq_stride, int N,
                                      int D, int d, int B, int Ld, const int32_t* d_pos2, const float* d_qkv_probe,
                                      int64_t probe_layer_stride, void* stream) {
  return kvcopy_debug("ttx_debug_kvcopy_split", s, d_rec, n_copy, d_qkv, qkv_layer_stride, d_kcache, d_vcache, cache_layer_stride,
                      cache_seq_stride, N, D, d, B, Ld, d_pos2, d_qkv_probe, probe_layer_stride, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int ttx_debug_kvcopy_select(ttx_session* s, const int32_t* d_rec, int n_copy, const float* d_qkv, int64_t qkv_layer_stride,
                                       float* d_kcache, float* d_vcache, int64_t cache_layer_stride, int64_t cache_seq_stride, int N,
                                       int D, int d, int B, int Ld, const int32_t* d_pos2, const float* d_qkv_probe,
                                       int64_t probe_layer_stride, const int32_t* d_row_base, const int32_t* d_draft_mask, void* stream) {
  if ((d_row_base != nullptr) != (d_draft_mask != nullptr))
    return fail(TTX_ERR_INVALID, "ttx_debug_kvcopy_select: row_base and draft_mask come together");
  return kvcopy_debug("ttx_debug_kvcopy_select", s, d_rec, n_copy, d_qkv, qkv_layer_stride, d_kcache, d_vcache, cache_layer_stride,
                      cache_seq_stride, N, D, d, B, Ld, d_pos2, d_qkv_probe, probe_layer_stride, reinterpret_cast<hipStream_t>(stream),
                      d_row_base, d_draft_mask);
}

// k_probe_split / k_merge_pred of the two-phase verify step (tests/test_gpu_two_phase.py).  The live count reaches the kernels as
// in production: in a DecState on the device.
static int dbg_state_with(hipStream_t st, int n_active, int steps, DecState** out) {
  DecState* dst = nullptr;
  HIP_TRY(hipMalloc((void**)&dst, 2 * sizeof(DecState)));
  DecState h[2] = {};
  h[0].n_active = n_active;
  h[1].steps = steps;
  const hipError_t e = hipMemcpy(dst, h, sizeof(h), hipMemcpyHostToDevice);
  (void)st;
  if (e != hipSuccess) { (void)hipFree(dst); HIP_TRY(e); }
  *out = dst;
  return TTX_OK;
}

// d_draft_mask / d_row_base / d_row_map (ttx_debug_probe_split_select; all null: ttx_debug_probe_split): result has 8 words then
static int probe_split_debug(ttx_session* s, const int32_t* d_act_idx, const int32_t* d_pred_probe, const int32_t* d_drafts,
                             int B, int N, int D, int n_active, int32_t* d_act2, int32_t* d_pos2, int32_t* result,
                             int32_t* d_draft_mask, int32_t* d_row_base, int32_t* d_row_map, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !d_act_idx || !d_pred_probe || !d_drafts || !d_act2 || !d_pos2 || !result)
    return fail(TTX_ERR_INVALID, "null argument to ttx_debug_probe_split");
  if (B < 1 || N < 1 || D < 1) return fail(TTX_ERR_INVALID, "ttx_debug_probe_split: B, N and D must be positive");
  if (n_active < 0 || n_active > B) return fail(TTX_ERR_INVALID, "ttx_debug_probe_split: n_active must lie in [0, B]");
  HIP_TRY(hipSetDevice(s->m->device));
  HIP_TRY(hipStreamSynchronize(st));
  if (n_active > 0) {
    std::vector<int> act((size_t)n_active);
    HIP_TRY(hipMemcpy(act.data(), d_act_idx, (size_t)n_active * 4, hipMemcpyDeviceToHost));
    std::vector<char> seen((size_t)B, 0);
    for (int b : act) {
      if (b < 0 || b >= B || seen[b]) return fail(TTX_ERR_INVALID, "ttx_debug_probe_split: act_idx must be distinct rows of [0, B)");
      seen[b] = 1;
    }
  }
  ProbeInfo* hinfo = nullptr;
  if (hipHostMalloc((void**)&hinfo, sizeof(ProbeInfo), hipHostMallocMapped) != hipSuccess) return fail(TTX_ERR_NOMEM, "hipHostMalloc failed");
  hinfo->matches = -1; hinfo->probes_done = -1; hinfo->rows = -1;
  DecState* dst = nullptr;
  int rc = dbg_state_with(st, n_active, result[4], &dst);           // result[4] on entry: probes counted so far
  int* d_exec = nullptr;
  hipError_t err = hipSuccess;
  if (rc == TTX_OK) err = hipMalloc((void**)&d_exec, 4);
  if (rc == TTX_OK && err == hipSuccess) {
    ProbeSplitArgs ps{};
    ps.st = dst; ps.act_idx = d_act_idx; ps.pred_probe = d_pred_probe; ps.drafts = d_drafts; ps.N = N; ps.D = D;
    ps.act2 = d_act2; ps.pos2 = d_pos2; ps.st2 = dst + 1; ps.exec_rows = d_exec;
    ps.draft_mask = d_draft_mask; ps.row_base = d_row_base; ps.row_map = d_row_map;
    err = hipHostGetDevicePointer((void**)&ps.host, (void*)hinfo, 0);
    if (err == hipSuccess) {
      hipLaunchKernelGGL(k_probe_split, dim3(1), dim3(B > 256 ? ACCEPT_THREADS : 256), 0, st, ps);
      err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    DecState h2{};
    int exec = 0;
    if (err == hipSuccess) err = hipMemcpy(&h2, dst + 1, sizeof(DecState), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(&exec, d_exec, 4, hipMemcpyDeviceToHost);
    if (err == hipSuccess) {
      result[0] = h2.n_active; result[1] = h2.r_rows; result[2] = h2.m_rows; result[3] = exec; result[4] = h2.steps;
      result[5] = hinfo->matches; result[6] = hinfo->probes_done;
      if (d_row_base) result[7] = hinfo->rows;
    }
  }
  if (d_exec) (void)hipFree(d_exec);
  if (dst) (void)hipFree(dst);
  (void)hipHostFree(hinfo);
  TTX_TRY(rc);
  HIP_TRY(err);
  return TTX_OK;
}

extern "C" int ttx_debug_probe_split(ttx_session* s, const int32_t* d_act_idx, const int32_t* d_pred_probe, const int32_t* d_drafts,
                                     int B, int N, int D, int n_active, int32_t* d_act2, int32_t* d_pos2, int32_t* result,
                                     void* stream) {
  return probe_split_debug(s, d_act_idx, d_pred_probe, d_drafts, B, N, D, n_active, d_act2, d_pos2, result, nullptr, nullptr, nullptr, stream);
}

extern "C" int ttx_debug_probe_split_select(ttx_session* s, const int32_t* d_act_idx, const int32_t* d_pred_probe, const int32_t* d_drafts,
                                            int B, int N, int D, int n_active, int32_t* d_act2, int32_t* d_pos2, int32_t* d_draft_mask,
                                            int32_t* d_row_base, int32_t* d_row_map, int32_t* result, void* stream) {
  if ((d_draft_mask != nullptr) != (d_row_base != nullptr) || (d_row_base != nullptr) != (d_row_map != nullptr))
    return fail(TTX_ERR_INVALID, "ttx_debug_probe_split_select: draft_mask, row_base and row_map come together");
  if (d_row_base && N > 32) return fail(TTX_ERR_INVALID, "ttx_debug_probe_split_select: draft select needs N <= 32");
  return probe_split_debug(s, d_act_idx, d_pred_probe, d_drafts, B, N, D, n_active, d_act2, d_pos2, result, d_draft_mask, d_row_base,
                           d_row_map, stream);
}

// d_row_base / d_draft_mask (ttx_debug_merge_pred_select; both null: ttx_debug_merge_pred): d_pred2 is compacted
static int merge_pred_debug(ttx_session* s, const int32_t* d_pos2, const int32_t* d_pred_probe, const int32_t* d_pred2,
                            int32_t* d_pred, int B, int N, int D, int n_active, const int32_t* d_row_base, const int32_t* d_draft_mask,
                            void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!s || !d_pos2 || !d_pred_probe || !d_pred2 || !d_pred) return fail(TTX_ERR_INVALID, "null argument to ttx_debug_merge_pred");
  if (B < 1 || N < 1 || D < 1) return fail(TTX_ERR_INVALID, "ttx_debug_merge_pred: B, N and D must be positive");
  if (n_active < 0 || n_active > B) return fail(TTX_ERR_INVALID, "ttx_debug_merge_pred: n_active must lie in [0, B]");
  HIP_TRY(hipSetDevice(s->m->device));
  HIP_TRY(hipStreamSynchronize(st));
  if (n_active > 0) {
    std::vector<int> pos((size_t)n_active);
    HIP_TRY(hipMemcpy(pos.data(), d_pos2, (size_t)n_active * 4, hipMemcpyDeviceToHost));
    for (int p : pos)
      if (p < -1 || p >= B) return fail(TTX_ERR_INVALID, "ttx_debug_merge_pred: pos2 must lie in [-1, B)");
    if (d_row_base || d_draft_mask) {
      int n_pos = 0, total = 0;
      for (int p : pos) n_pos = std::max(n_pos, p + 1);
      TTX_TRY(dbg_check_select("ttx_debug_merge_pred_select", d_row_base, d_draft_mask, n_pos, N, D, st, nullptr, &total));
    }
  }
  DecState* dst = nullptr;
  TTX_TRY(dbg_state_with(st, n_active, 0, &dst));
  MergePredArgs mp{};
  mp.st = dst; mp.pos2 = d_pos2; mp.pred_probe = d_pred_probe; mp.pred2 = d_pred2; mp.pred = d_pred; mp.RPS = step_rps(N, D);
  mp.row_base = d_row_base; mp.draft_mask = d_draft_mask; mp.D = D;
  hipLaunchKernelGGL(k_merge_pred, dim3(cdiv(B * mp.RPS, 256)), dim3(256), 0, st, mp);
  hipError_t err = hipGetLastError();
  const hipError_t esync = hipStreamSynchronize(st);
  (void)hipFree(dst);
  HIP_TRY(err);
  HIP_TRY(esync);
  return TTX_OK;
}

extern "C" int ttx_debug_merge_pred(ttx_session* s, const int32_t* d_pos2, const int32_t* d_pred_probe, const int32_t* d_pred2,
                                    int32_t* d_pred, int B, int N, int D, int n_active, void* stream) {
  return merge_pred_debug(s, d_pos2, d_pred_probe, d_pred2, d_pred, B, N, D, n_active, nullptr, nullptr, stream);
}

extern "C" int ttx_debug_merge_pred_select(ttx_session* s, const int32_t* d_pos2, const int32_t* d_pred_probe, const int32_t* d_pred2,
                                           int32_t* d_pred, int B, int N, int D, int n_active, const int32_t* d_row_base,
                                           const int32_t* d_draft_mask, void* stream) {
  if ((d_row_base != nullptr) != (d_draft_mask != nullptr))
    return fail(TTX_ERR_INVALID, "ttx_debug_merge_pred_select: row_base and draft_mask come together");
  return merge_pred_debug(s, d_pos2, d_pred_probe, d_pred2, d_pred, B, N, D, n_active, d_row_base, d_draft_mask, stream);
}

extern "C" int ttx_pool_last_counters(ttx_session* s, int64_t* counters) {
  if (!s || !counters) return fail(TTX_ERR_INVALID, "null argument to ttx_pool_last_counters");
  for (int i = 0; i < 7; ++i) counters[i] = s->pool_counters[i];
  return TTX_OK;
}

extern "C" int ttx_attn_staged_key_limit(int head_dim, int q_per_group) { return attn_staged_key_limit(head_dim, q_per_group); }

extern "C" int ttx_debug_attn_kernels_seen(ttx_session* s) {
  if (!s) return fail(TTX_ERR_INVALID, "null session");
  return (int)s->attn_kernels_seen;
}

extern "C" int ttx_last_kernel_profile(ttx_session* s, double* gemm_ms, int64_t* gemm_launches, double* empty_pair_ms) {
  if (!s) return fail(TTX_ERR_INVALID, "null session");
  if (gemm_ms) *gemm_ms = s->prof_ms;
  if (gemm_launches) *gemm_launches = s->prof_launches;
  s->prof_ms = 0;
  s->prof_launches = 0;
  if (empty_pair_ms) *empty_pair_ms = s->prof_empty_pair_ms < 0 ? 0.0 : s->prof_empty_pair_ms;
  return TTX_OK;
}
