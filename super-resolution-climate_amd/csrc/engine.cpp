// srmi engine: the RCAN / EDSR network plan, workspace layout and the
// forward / backward / optimizer orchestration behind the C ABI of
// include/srmi.h.  Every launch is asynchronous on the caller's stream; the
// engine never synchronises and allocates nothing (graph-capturable).
//
// Network structure follows the reference exactly:
//   RCAN  sres/model/rcan/network.py:7-77, blocks.py:58-76
//   EDSR  sres/model/edsr/network.py:9-32, common/residual.py:26-50,
//         common/upsample.py:32-66
// Parameter order = the reference state_dict order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "srmi_internal.hpp"

using namespace srmi;

namespace {

struct ConvRef {
  long long w = -1, b = -1;  // param offsets
  int cin = 0, cout = 0, ps = 0;
  long long f_off = -1, d_off = -1, pb_off = -1;  // pack offsets (MFMA convs only)
};

struct RCABRef {
  ConvRef c1, c2;
  long long ca_w1, ca_b1, ca_w2, ca_b2;
};

struct Plan {
  srmi_model_config cfg;
  std::vector<srmi_param_info> params;
  long long n_params = 0;
  ConvRef head, body_tail, tail;
  std::vector<std::vector<RCABRef>> groups;  // RCAN
  std::vector<ConvRef> group_tail;            // RCAN
  std::vector<ConvRef> res1, res2;            // EDSR
  std::vector<ConvRef> ups;
  std::vector<ConvRef*> mfma_convs;
  long long pack_elems = 0, pbias_elems = 0;
  int nups = 0;
};

long long add_param(Plan& P, std::initializer_list<int> shape) {
  srmi_param_info pi{};
  pi.offset = P.n_params;
  pi.ndim = (int)shape.size();
  long long n = 1;
  int k = 0;
  for (int s : shape) {
    pi.shape[k++] = s;
    n *= s;
  }
  pi.numel = n;
  P.params.push_back(pi);
  P.n_params += n;
  return pi.offset;
}

ConvRef add_conv(Plan& P, int cin, int cout, int k) {
  ConvRef c;
  c.cin = cin;
  c.cout = cout;
  c.w = add_param(P, {cout, cin, k, k});
  c.b = add_param(P, {cout});
  return c;
}

int build_plan(const srmi_model_config* cfg, Plan& P) {
  if (!cfg) return SRMI_ERR_ARG;
  const srmi_model_config& c = *cfg;
  if (c.nfeatures != 64) return SRMI_ERR_UNSUPPORTED;
  if (c.nchannels_in < 1 || c.nchannels_in > 4 || c.nchannels_out < 1 || c.nchannels_out > 4) return SRMI_ERR_UNSUPPORTED;
  if (c.scale != 2 && c.scale != 4 && c.scale != 8) return SRMI_ERR_UNSUPPORTED;
  if (c.nlayers < 1 || c.batch < 1 || c.lr_h < 4 || c.lr_w < 16) return SRMI_ERR_ARG;
  if (c.arch == SRMI_ARCH_RCAN && (c.nblocks < 1 || c.reduction < 1 || 64 % c.reduction)) return SRMI_ERR_ARG;
  // the CA kernels take CR = 64 / reduction in 4 .. 32, a multiple of 4 (records sized for 32):
  // refused here rather than at the first CA launch
  if (c.arch == SRMI_ARCH_RCAN && (64 / c.reduction > 32 || (64 / c.reduction) % 4)) return SRMI_ERR_UNSUPPORTED;
  if (c.arch != SRMI_ARCH_RCAN && c.arch != SRMI_ARCH_EDSR) return SRMI_ERR_ARG;
  if (c.dtype != SRMI_DTYPE_BF16 && c.dtype != SRMI_DTYPE_F32) return SRMI_ERR_ARG;
  if (c.flags & ~(SRMI_FLAG_NO_RCAB_INFER | SRMI_FLAG_CA_PASS | SRMI_FLAG_DU_PASS)) return SRMI_ERR_ARG;  // (retired bits refused)
  P = Plan();
  P.cfg = c;
  const int F = 64;
  P.head = add_conv(P, c.nchannels_in, F, 3);
  if (c.arch == SRMI_ARCH_RCAN) {
    P.groups.resize(c.nlayers);
    for (int g = 0; g < c.nlayers; ++g) {
      for (int b = 0; b < c.nblocks; ++b) {
        RCABRef r;
        r.c1 = add_conv(P, F, F, 3);
        r.c2 = add_conv(P, F, F, 3);
        r.ca_w1 = add_param(P, {F / c.reduction, F, 1, 1});
        r.ca_b1 = add_param(P, {F / c.reduction});
        r.ca_w2 = add_param(P, {F, F / c.reduction, 1, 1});
        r.ca_b2 = add_param(P, {F});
        P.groups[g].push_back(r);
      }
      P.group_tail.push_back(add_conv(P, F, F, 3));
    }
  } else {
    for (int i = 0; i < c.nlayers; ++i) {
      P.res1.push_back(add_conv(P, F, F, 3));
      P.res2.push_back(add_conv(P, F, F, 3));
    }
  }
  P.body_tail = add_conv(P, F, F, 3);
  P.nups = (int)std::lround(std::log2((double)c.scale));
  for (int k = 0; k < P.nups; ++k) {
    ConvRef u = add_conv(P, F, 4 * F, 3);
    u.ps = 1;
    P.ups.push_back(u);
  }
  P.tail = add_conv(P, F, c.nchannels_out, 3);
  // MFMA convs get filter packs in the operand type (bf16 or fp32)
  for (auto& grp : P.groups)
    for (auto& r : grp) {
      P.mfma_convs.push_back(&r.c1);
      P.mfma_convs.push_back(&r.c2);
    }
  for (auto& t : P.group_tail) P.mfma_convs.push_back(&t);
  for (size_t i = 0; i < P.res1.size(); ++i) {
    P.mfma_convs.push_back(&P.res1[i]);
    P.mfma_convs.push_back(&P.res2[i]);
  }
  P.mfma_convs.push_back(&P.body_tail);
  for (auto& u : P.ups) P.mfma_convs.push_back(&u);
  for (ConvRef* cr : P.mfma_convs) {
    const long long n = (long long)cr->cout * cr->cin * 9;
    cr->f_off = P.pack_elems;
    P.pack_elems += n;
    cr->d_off = P.pack_elems;
    P.pack_elems += n;
    cr->pb_off = P.pbias_elems;
    P.pbias_elems += cr->cout;
  }
  return 0;
}

// ---------------------------------------------------------------- workspace
struct Carver {
  size_t off = 0;
  char* base = nullptr;
  template <class T>
  T* take(size_t count) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};

int choose_row_splits(int N, int H, int Cout, int cu_budget = 0) {
  // wgrad grid = N*rs chunks x Cout/64 (one workgroup per CU by LDS); aim at >= 3/4
  // of the CU budget while keeping as few partial slabs (N*rs) as possible; rows per
  // chunk % 4 == 0
  const int target = 3 * (cu_budget > 0 ? cu_budget : 256) / 4;
  int best = 1;
  for (int rs = 1; rs <= H / 4; ++rs) {
    if (H % rs || (H / rs) % 4) continue;
    best = rs;
    if (N * rs * (Cout / 64) >= target) break;
  }
  return best;
}

}  // namespace

struct srmi_engine {
  Plan P;
  int train = 0;
  // operand storage: bf16 (SRMI_DTYPE_BF16: bf16 MFMA operands, fp32 accumulation
  // and residual stream) or fp32 (SRMI_DTYPE_F32: exact fp32 everywhere).  The
  // activation / gradient-map / filter-pack pointers below are typed bf16_t* but
  // hold esz-byte elements; at() does their element arithmetic.
  int f32 = 0;
  size_t esz = 2;
  int N = 0, h = 0, w = 0, C = 0, Co = 0, S = 0;
  int cu_budget = 0;  // CUs one launch aims to fill (0 = all)
  size_t mapn = 0;  // elements of one [N][h][w][64] map
  // forward state
  float *X0f, *Rf, *Hf;
  bf16_t* HB;    // hb maps
  int n_hb;      // number of hb slots
  bf16_t *T, *U; // train: [nl*nb] maps; infer: 1 each
  bf16_t* RESb;
  bf16_t* PS[3];  // pixel-shuffle outputs (scale s: [N][h*2^k][w*2^k][64])
  float *rec, *brec;
  float *ppool, *pacc;
  float* mpart;  // conv1's partial CA means [N][runs per image <= nstrips][64]
  // backward
  float *GAf, *GBf, *dRESf;
  bf16_t *GAb, *GBb, *DU, *DZ, *dRESb;
  bf16_t* dPS[3];
  float *slab, *bslab;
  size_t slab_floats, bslab_floats;
  // the RCAB filter gradients' slab sets of one residual group: set (b, c) = RCAB b's conv2
  // (c = 0) / conv1 (c = 1) filter gradient, b = 1 .. nblocks; (0, 0) the group tail's.  One
  // per launch, so the reductions can wait for the group's end (one launch for all)
  std::vector<float*> slab_sets, bslab_sets;
  size_t slab_r_floats = 0, bslab_r_floats = 0;
  float* slab_r(int b, int c) const { return slab_sets[b * 2 + c]; }
  float* bslab_r(int b, int c) const { return bslab_sets[b * 2 + c]; }
  float* lpart;
  int lpart_n;
  float* zeros;  // 256 zero bytes (DMA padding source)
  // packs
  bf16_t* packs;
  float* pbias;
  PackEntry* d_entries;
  long long* d_caoffs;
  std::vector<PackEntry> h_entries;
  std::vector<long long> h_caoffs;
  int max_cob = 0, max_cib = 0;  // largest Cout / 64, Cin / 64 of the packed convs
  bool tables_uploaded = false;
  int last_n = 0;
  // the backward stage srmi_backward_stages must run next (0 after a forward or a
  // completed backward): the gradient-stream buffers and the slab parity carry over
  // from one stage to the next, so a skipped, repeated or reordered stage is refused
  int next_stage = 0;
  const float* probe_prm = nullptr;  // the parameters of the last backward / inference forward (srmi_engine_probe)
  // diagnostic (srmi_engine_trace): the caller's buffer the RCAN backward copies its in-group
  // state into, one region per residual group; null = off (one branch per copy site)
  char* trace = nullptr;
  // diagnostic (srmi_engine_fwd_trace): the same for the bf16 RCAN forward's transient state
  char* ftrace = nullptr;

  bf16_t* at(bf16_t* base, size_t elems) const {
    return reinterpret_cast<bf16_t*>(reinterpret_cast<char*>(base) + elems * esz);
  }
  bf16_t* hb(int g, int b) const {
    const int nb1 = P.cfg.arch == SRMI_ARCH_RCAN ? P.cfg.nblocks + 1 : 1;
    const int k = g * nb1 + b;
    return at(HB, (size_t)(train ? k : (k % n_hb)) * mapn);
  }
  int nbe() const { return P.cfg.arch == SRMI_ARCH_RCAN ? P.cfg.nblocks : 1; }
  bf16_t* Tm(int g, int b) const { return train ? at(T, (size_t)(g * nbe() + (b - 1)) * mapn) : T; }
  bf16_t* Um(int g, int b) const { return train ? at(U, (size_t)(g * P.cfg.nblocks + (b - 1)) * mapn) : U; }
  float* recp(int g, int b) const {
    return train ? rec + (size_t)(g * P.cfg.nblocks + (b - 1)) * N * 160 : rec;
  }
  float* brecp(int g, int b) const { return brec + (size_t)(g * P.cfg.nblocks + (b - 1)) * N * 224; }
};

// The RCAB filter gradients run beside their dgrad convs (one fused launch, the
// CU budget split in halves), so their row chunks are sized for HALF the engine's
// budget: fewer, longer chunks write fewer partial slabs (at C2 2 x 24-row chunks
// per image instead of 3 x 16).
static int engine_cus(const srmi_engine* e) { return e->cu_budget > 0 ? e->cu_budget : 256; }
// CU shares of the two parts of a fused launch, in percent of the engine budget taken
// by the filter gradient: after the ReLU-mask dgrad of conv2 (FUSE_WG2) and after the
// gradient-accumulating dgrad of conv1 (FUSE_WG1, the heavier conv epilogue)
static int fuse_wg_cus(const srmi_engine* e, int which) {
  (void)which;  // half the budget for both fused launches (44 / 56 % measured within noise)
  return engine_cus(e) / 2;
}
static int rcab_row_splits(const srmi_engine* e, int n, int which) {
  return choose_row_splits(n, e->h, 64, fuse_wg_cus(e, which));
}

static size_t carve(srmi_engine* e, char* base) {
  Carver cv;
  cv.base = base;
  auto act = [&](size_t count) { return reinterpret_cast<bf16_t*>(cv.take<char>(count * e->esz)); };
  const Plan& P = e->P;
  const int N = e->N;
  const size_t m = e->mapn;
  const bool rcan = P.cfg.arch == SRMI_ARCH_RCAN;
  const int nl = P.cfg.nlayers, nb = rcan ? P.cfg.nblocks : 0;
  e->X0f = cv.take<float>(m);
  e->Rf = cv.take<float>(m);
  e->Hf = cv.take<float>(m);
  const int nslots = rcan ? nl * (nb + 1) + 1 : nl + 1;
  e->n_hb = e->train ? nslots : 3;
  e->HB = act(m * e->n_hb);
  const int nconv1 = rcan ? nl * nb : nl;
  e->T = act(m * (e->train ? nconv1 : 1));
  e->U = rcan ? act(m * (e->train ? nconv1 : 1)) : nullptr;
  e->RESb = act(m);
  for (int k = 0; k < 3; ++k) e->PS[k] = nullptr;
  for (int k = 0; k < P.nups; ++k) e->PS[k] = act(m << (2 * (k + 1)));
  const int nstrips = conv3x3_nstrips(e->h, e->w);
  if (rcan) {
    e->rec = cv.take<float>((size_t)(e->train ? nl * nb : 1) * N * 160);
    e->brec = e->train ? cv.take<float>((size_t)nl * nb * N * 224) : nullptr;  // [N][160] + dm[N][64]
    e->ppool = cv.take<float>((size_t)N * nstrips * 64);
    e->mpart = e->train ? cv.take<float>((size_t)N * nstrips * 64) : nullptr;
    e->pacc = cv.take<float>((size_t)N * nstrips * 128);
  }
  e->lpart_n = 1024;
  e->lpart = cv.take<float>(e->lpart_n);
  e->zeros = cv.take<float>(64);
  if (e->train) {
    e->GAf = cv.take<float>(m);
    e->GBf = cv.take<float>(m);
    e->dRESf = cv.take<float>(m);
    e->GAb = act(m);
    e->GBb = act(m);
    e->DU = act(m);
    e->DZ = act(m);
    e->dRESb = act(m);
    for (int k = 0; k < 3; ++k) e->dPS[k] = nullptr;
    for (int k = 0; k < P.nups; ++k) e->dPS[k] = act(m << (2 * (k + 1)));
    // slab: max over all wgrads
    size_t sf = 0, bf = 0;
    auto upd = [&](int H, int W, int Cout) {
      // a call may pass fewer tiles than the capacity (a short last batch), and
      // fewer tiles get more row splits: size for the largest n * rs(n)
      for (int n = 1; n <= N; ++n) {
        const size_t ns = (size_t)n * choose_row_splits(n, H, Cout, e->cu_budget) * (W % 48 == 0 ? W / 48 : 1);
        sf = std::max(sf, ns * Cout * 576);
        bf = std::max(bf, ns * Cout);
      }
    };
    upd(e->h, e->w, 64);
    for (int k = 0; k < P.nups; ++k) upd(e->h << k, e->w << k, 256);
    // head / tail slabs
    const int Hs = e->h * e->S;
    sf = std::max(sf, (size_t)N * (e->h / 2) * 64 * (9 * e->C + 1));  // head wgrad: 2-row bands
    sf = std::max(sf, (size_t)N * (Hs / 4) * e->Co * 577);  // tail_wgrad: 4-row bands
    e->slab_floats = sf;
    e->bslab_floats = bf;
    e->slab = cv.take<float>(sf);
    e->bslab = cv.take<float>(bf);
    if (rcan) {  // the RCAB filter-gradient slab sets (64-channel convs only)
      size_t ns = 0;  // (wgrad48: a slab per 48-wide column tile too, as wgrad3x3_nslabs counts)
      for (int n = 1; n <= N; ++n)
        ns = std::max(ns, (size_t)n * std::max(rcab_row_splits(e, n, 1), rcab_row_splits(e, n, 2)) *
                              (e->w % 48 == 0 ? e->w / 48 : 1));
      e->slab_r_floats = ns * 64 * 576;
      e->bslab_r_floats = ns * 64;
      const int nsets = (P.cfg.nblocks + 1) * 2;  // (slab_r)
      e->slab_sets.assign(nsets, nullptr);
      e->bslab_sets.assign(nsets, nullptr);
      for (int i = 0; i < nsets; ++i) {
        if (i == 1) continue;  // (the group tail has one filter gradient)
        e->slab_sets[i] = cv.take<float>(e->slab_r_floats);
        e->bslab_sets[i] = cv.take<float>(e->bslab_r_floats);
      }
    }
  }
  e->packs = act(P.pack_elems);
  e->pbias = cv.take<float>(P.pbias_elems);
  e->d_entries = cv.take<PackEntry>(P.mfma_convs.size());
  e->d_caoffs = cv.take<long long>((size_t)std::max(1, nl * nb) * 5);
  return cv.off + 256;
}

static int init_engine(srmi_engine* e, const srmi_model_config* cfg, int train) {
  int rc = build_plan(cfg, e->P);
  if (rc) return rc;
  e->train = train;
  e->f32 = cfg->dtype == SRMI_DTYPE_F32;
  e->esz = e->f32 ? 4 : 2;
  e->N = cfg->batch;
  e->h = cfg->lr_h;
  e->w = cfg->lr_w;
  e->C = cfg->nchannels_in;
  e->Co = cfg->nchannels_out;
  e->S = cfg->scale;
  e->cu_budget = cfg->cu_budget > 0 ? cfg->cu_budget : 0;
  e->mapn = (size_t)e->N * e->h * e->w * 64;
  if (e->h % 4 || (e->w % 32 && e->w % 48)) return SRMI_ERR_SHAPE;
  const int Hs = e->h * e->S;
  if (Hs % 16 || ((e->w * e->S) % 32)) return SRMI_ERR_SHAPE;
  // the kernels store activation / gradient maps through buffer resources with a
  // 32-bit byte range: refuse any map of 2^32 bytes or more (the largest is the
  // last pixel-shuffle output, mapn << 2 nups elements, and the fp32 streams)
  const size_t lim = (size_t)1 << 32;
  const size_t ps_bytes = (e->mapn << (2 * e->P.nups)) * e->esz;
  const size_t f32_bytes = e->mapn * 4;
  const size_t hr_bytes = (size_t)e->N * std::max(e->C, e->Co) * Hs * (e->w * e->S) * 4;
  if (ps_bytes >= lim || f32_bytes >= lim || hr_bytes >= lim) return SRMI_ERR_SHAPE;
  return 0;
}

static void build_tables(srmi_engine* e) {
  e->h_entries.clear();
  e->max_cob = e->max_cib = 0;
  for (ConvRef* c : e->P.mfma_convs) {
    PackEntry pe{};
    pe.w_off = c->w;
    pe.b_off = c->b;
    pe.f_off = c->f_off;
    pe.d_off = c->d_off;
    pe.pb_off = c->pb_off;
    pe.Cout = c->cout;
    pe.Cin = c->cin;
    pe.ps = c->ps;
    e->h_entries.push_back(pe);
    e->max_cob = std::max(e->max_cob, (c->cout + 63) / 64);
    e->max_cib = std::max(e->max_cib, (c->cin + 63) / 64);
  }
  e->h_caoffs.clear();
  for (auto& grp : e->P.groups)
    for (auto& r : grp) {
      e->h_caoffs.push_back(r.ca_w1);
      e->h_caoffs.push_back(r.ca_b1);
      e->h_caoffs.push_back(r.ca_w2);
      e->h_caoffs.push_back(r.ca_b2);
      e->h_caoffs.push_back(r.c2.b);
    }
}

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

// --------------------------------------------------------------- conv helpers
// forward convs sized for this share of the engine's CU budget (A/B: fewer, longer runs)
static ConvParams fwd_params(srmi_engine* e, const ConvRef& c, const bf16_t* x, int n, int H, int W, bf16_t* yb,
                             float* yf, const float* r1, float* part, float alpha) {
  ConvParams p{};
  p.x = x;
  p.w = e->at(e->packs, c.f_off);
  p.bias = e->pbias + c.pb_off;
  p.f32 = e->f32;
  p.N = n;
  p.H = H;
  p.W = W;
  p.Cin = c.cin;
  p.Cout = c.cout;
  p.in_mode = IN_PLAIN;
  p.yb = yb;
  p.yf = yf;
  p.r1 = r1;
  p.part = part;
  p.part_stride = 64;
  p.alpha = alpha;
  p.zeros = e->zeros;
  p.cu_budget = e->cu_budget;
  return p;
}

static int conv_fwd(srmi_engine* e, const ConvRef& c, const bf16_t* x, int n, int H, int W, int epi, bf16_t* yb,
                    float* yf, const float* r1, float* part, float alpha, hipStream_t st) {
  return conv3x3_launch(fwd_params(e, c, x, n, H, W, yb, yf, r1, part, alpha), epi, st);
}

// dgrad of conv c: input dy (Cout channels, PS layout if c.ps), output Cin channels
static ConvParams dgrad_params(srmi_engine* e, const ConvRef& c, const bf16_t* dy, int n, int H, int W, int* epi,
                               bf16_t* yb, float* yf, const float* r1, const float* r2, const float* r3,
                               const bf16_t* aux, float* part, float alpha, const bf16_t* r1b = nullptr) {
  ConvParams p{};
  p.x = dy;
  p.w = e->at(e->packs, c.d_off);
  p.bias = nullptr;
  p.f32 = e->f32;
  p.N = n;
  p.H = H;
  p.W = W;
  p.Cin = c.cout;
  p.Cout = c.cin;
  p.in_mode = c.ps ? IN_UNSHUF : IN_PLAIN;
  p.yb = yb;
  p.yf = yf;
  p.r1 = r1;
  p.r1b = r1b;
  p.r2 = r2;
  p.r3 = r3;
  p.aux = aux;
  p.part = part;
  p.part_stride = 128;
  p.alpha = alpha;
  p.zeros = e->zeros;
  p.cu_budget = e->cu_budget;
  // the hot RCAB cases: specialised epilogues without runtime operand checks
  if (*epi == EPI_DG_ACC && r1 && aux && part && !yb && !r2 && !r3 && yf && c.cout == 64 && !c.ps)
    *epi = EPI_DG_ACC_CA;
  if (*epi == EPI_DG_ACC && r1b && !r1 && aux && part && yb && !r2 && !r3 && !yf && c.cout == 64 && !c.ps)
    *epi = EPI_DG_ACC_CA16;  // (the bf16 engine's in-group gradient stream)
  if (*epi == EPI_DG_ACC && !r1b && !r1 && aux && part && yb && !r2 && !r3 && !yf && c.cout == 64 && !c.ps)
    *epi = EPI_DG_CA16;  // (the group tail's dgrad: the stream's start)
  if (*epi == EPI_DG_ACC && r1b && !r1 && !aux && !part && yb && yf && r2 && c.cout == 64 && !c.ps)
    *epi = EPI_DG_ACC_G1;  // (the group's first RCAB: the stream's end)
  return p;
}

static int conv_dgrad(srmi_engine* e, const ConvRef& c, const bf16_t* dy, int n, int H, int W, int epi, bf16_t* yb,
                      float* yf, const float* r1, const float* r2, const float* r3, const bf16_t* aux, float* part,
                      float alpha, hipStream_t st) {
  ConvParams p = dgrad_params(e, c, dy, n, H, W, &epi, yb, yf, r1, r2, r3, aux, part, alpha);
  return conv3x3_launch(p, epi, st);
}

// filter gradient of conv c into `slab`/`bslab` (capacity cap/bcap floats); the
// reduction into grads is returned in *red.  slab16: bf16 partial slabs, the RCAB filter
// gradients'.  The other filter gradients (group / body tails, upsamplers: 26 launches per
// step) keep fp32 slabs: bf16 there measured +0.3 % (noise) and doubled the split dependence
// of their sums (one engine of 16 tiles vs 2 x 2 engines of 4: 2.4e-4 rel-L2 of the gradient)
static int wgrad_params(srmi_engine* e, const ConvRef& c, const bf16_t* x, const bf16_t* dy, int n, int H, int W,
                        float* grads, bool with_bias, float alpha, int row_splits, float* slab, float* bslab,
                        size_t cap, size_t bcap, WgradParams* out, ReduceSet* red, bool slab16 = false) {
  WgradParams p{};
  p.x = x;
  p.dy = dy;
  p.f32 = e->f32;
  p.N = n;
  p.H = H;
  p.W = W;
  p.Cout = c.cout;
  p.dy_mode = c.ps ? IN_UNSHUF : IN_PLAIN;
  p.imgs_per_wg = 1;
  p.row_splits = row_splits;
  p.slab = slab;
  p.bslab = bslab;
  p.zeros = e->zeros;
  // bf16 weight slabs only where the wgrad48 body writes them (layout 1)
  p.slab16 = slab16 && !e->f32 && wgrad3x3_slab_layout(p) == 1;
  const size_t ns = (size_t)wgrad3x3_nslabs(p);
  if (ns * c.cout * 576 > cap || ns * c.cout > bcap) return SRMI_ERR_WORKSPACE;
  *out = p;
  *red = ReduceSet{p.slab, p.bslab, (int)ns, c.cout, c.ps, wgrad3x3_slab_layout(p), alpha, grads + c.w,
                   with_bias ? grads + c.b : nullptr, p.slab16};
  return 0;
}

// filter gradient + its reduction, both on st (upsampler / group-tail / body-tail /
// EDSR convs)
static int conv_wgrad(srmi_engine* e, const ConvRef& c, const bf16_t* x, const bf16_t* dy, int n, int H, int W,
                      float* grads, bool with_bias, float alpha, hipStream_t st) {
  WgradParams p;
  ReduceSet r;
  const int rc = wgrad_params(e, c, x, dy, n, H, W, grads, with_bias, alpha, choose_row_splits(n, H, c.cout, e->cu_budget),
                              e->slab, e->bslab, e->slab_floats, e->bslab_floats, &p, &r);
  if (rc) return rc;
  const int rc2 = wgrad3x3_launch(p, st);
  if (rc2) return rc2;
  return wgrad_reduce_launch(r.slab, r.bslab, r.nslab, r.Cout, r.ps, r.layout, r.alpha, r.gw, r.gb, st, r.slab16);
}

// a dgrad conv and the filter gradient of the same conv (independent, both reading
// dy): one fused launch where the shapes allow (bf16, 48-wide tiles), else the two
// launches one after the other on the same stream
static int dgrad_with_wgrad(srmi_engine* e, const ConvParams& cp, int epi, const WgradParams& wp, int which,
                            hipStream_t st) {
  if (rcab_bwd_fusable(cp, wp)) return rcab_bwd_launch(cp, epi, engine_cus(e) - fuse_wg_cus(e, which), wp, st);
  const int rc = wgrad3x3_launch(wp, st);
  if (rc) return rc;
  return conv3x3_launch(cp, epi, st);
}

// ---- the backward trace (srmi_engine_trace): layout of the caller's buffer.  Per residual
// group g, 256-byte aligned pieces in this order: GRB | STREAM b = 0 .. nb | PACC b = 1 .. nb |
// DZ b = 1 .. nb | DU b = 1 .. nb; maps are [N][h][w][64] of the engine's operand type (capacity
// N: the first n images are copied), PACC is fp32 [N][nstrips][128].
static size_t trace_map_bytes(const srmi_engine* e) { return (e->mapn * e->esz + 255) & ~(size_t)255; }
static size_t trace_pacc_bytes(const srmi_engine* e) {
  return ((size_t)e->N * conv3x3_nstrips(e->h, e->w) * 128 * sizeof(float) + 255) & ~(size_t)255;
}
static size_t trace_group_bytes(const srmi_engine* e) {
  const size_t nb = (size_t)e->P.cfg.nblocks;
  return trace_map_bytes(e) * (3 * nb + 2) + trace_pacc_bytes(e) * nb;
}
static size_t trace_bytes(const srmi_engine* e) { return trace_group_bytes(e) * (size_t)e->P.cfg.nlayers; }
// byte offset of slot (which, g, b), or (size_t)-1 if there is no such slot
static size_t trace_offset(const srmi_engine* e, int which, int g, int b) {
  const int nl = e->P.cfg.nlayers, nb = e->P.cfg.nblocks;
  if (g < 0 || g >= nl) return (size_t)-1;
  const size_t m = trace_map_bytes(e), pa = trace_pacc_bytes(e), base = trace_group_bytes(e) * (size_t)g;
  switch (which) {
    case SRMI_TRACE_GRB:
      return b == 0 ? base : (size_t)-1;
    case SRMI_TRACE_STREAM:
      return b >= 0 && b <= nb ? base + m * (size_t)(1 + b) : (size_t)-1;
    case SRMI_TRACE_PACC:
      return b >= 1 && b <= nb ? base + m * (size_t)(nb + 2) + pa * (size_t)(b - 1) : (size_t)-1;
    case SRMI_TRACE_DZ:
      return b >= 1 && b <= nb ? base + m * (size_t)(nb + 2) + pa * (size_t)nb + m * (size_t)(b - 1) : (size_t)-1;
    case SRMI_TRACE_DU:
      return b >= 1 && b <= nb ? base + m * (size_t)(2 * nb + 2) + pa * (size_t)nb + m * (size_t)(b - 1)
                               : (size_t)-1;
    default:
      return (size_t)-1;
  }
}
// one async device-to-device copy of the first n images' share of src into the slot
static int trace_copy(const srmi_engine* e, int which, int g, int b, const void* src, int n, hipStream_t st) {
  const size_t off = trace_offset(e, which, g, b);
  if (off == (size_t)-1) return SRMI_ERR_ARG;
  const size_t bytes = which == SRMI_TRACE_PACC ? (size_t)n * conv3x3_nstrips(e->h, e->w) * 128 * sizeof(float)
                                                : (size_t)n * e->h * e->w * 64 * e->esz;
  const hipError_t err = hipMemcpyAsync(e->trace + off, src, bytes, hipMemcpyDeviceToDevice, st);
  return err == hipSuccess ? 0 : -(int)err;
}

// ---- the forward trace (srmi_engine_fwd_trace): layout of the caller's buffer.  Per residual
// group g, 256-byte aligned pieces in this order: LO b = 1 .. nb | PPOOL b = 1 .. nb | RF, and for
// inference engines (whose hb / t / record slots rotate) HB b = 0 .. nb | T b = 1 .. nb | REC b =
// 1 .. nb; after the last group an inference engine's HB(nlayers, 0).  LO is [N][h][w][64] bytes,
// PPOOL fp32 [N][nstrips][64], RF an fp32 map, HB / T bf16 maps, REC fp32 [N][160] (capacity N:
// the first n images' share is copied).
static size_t ftrace_align(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t ftrace_piece_bytes(const srmi_engine* e, int which, int n) {
  const size_t px = (size_t)n * e->h * e->w * 64;
  switch (which) {
    case SRMI_FTRACE_LO: return px;
    case SRMI_FTRACE_PPOOL: return (size_t)n * conv3x3_nstrips(e->h, e->w) * 64 * sizeof(float);
    case SRMI_FTRACE_RF: return px * sizeof(float);
    case SRMI_FTRACE_REC: return (size_t)n * 160 * sizeof(float);
    default: return px * 2;  // HB, T
  }
}
static size_t ftrace_slot_bytes(const srmi_engine* e, int which) {
  return ftrace_align(ftrace_piece_bytes(e, which, e->N));
}
static size_t ftrace_group_bytes(const srmi_engine* e) {
  const size_t nb = (size_t)e->P.cfg.nblocks;
  size_t b = (ftrace_slot_bytes(e, SRMI_FTRACE_LO) + ftrace_slot_bytes(e, SRMI_FTRACE_PPOOL)) * nb +
             ftrace_slot_bytes(e, SRMI_FTRACE_RF);
  if (!e->train)
    b += ftrace_slot_bytes(e, SRMI_FTRACE_HB) * (nb + 1) +
         (ftrace_slot_bytes(e, SRMI_FTRACE_T) + ftrace_slot_bytes(e, SRMI_FTRACE_REC)) * nb;
  return b;
}
static size_t ftrace_bytes(const srmi_engine* e) {
  return ftrace_group_bytes(e) * (size_t)e->P.cfg.nlayers + (e->train ? 0 : ftrace_slot_bytes(e, SRMI_FTRACE_HB));
}
// the bf16 RCAN engines have this state (the exact-fp32 engine keeps no pair, EDSR no CA)
static bool ftrace_engine(const srmi_engine* e) { return e && !e->f32 && e->P.cfg.arch == SRMI_ARCH_RCAN; }
// byte offset of slot (which, g, b), or (size_t)-1 if there is no such slot
static size_t ftrace_offset(const srmi_engine* e, int which, int g, int b) {
  const int nl = e->P.cfg.nlayers, nb = e->P.cfg.nblocks;
  if (!e->train && which == SRMI_FTRACE_HB && g == nl && b == 0) return ftrace_group_bytes(e) * (size_t)nl;
  if (g < 0 || g >= nl) return (size_t)-1;
  const size_t lo = ftrace_slot_bytes(e, SRMI_FTRACE_LO), pp = ftrace_slot_bytes(e, SRMI_FTRACE_PPOOL),
               rf = ftrace_slot_bytes(e, SRMI_FTRACE_RF), hbb = ftrace_slot_bytes(e, SRMI_FTRACE_HB),
               tb = ftrace_slot_bytes(e, SRMI_FTRACE_T), rc = ftrace_slot_bytes(e, SRMI_FTRACE_REC);
  const size_t base = ftrace_group_bytes(e) * (size_t)g, inf = base + (lo + pp) * (size_t)nb + rf;
  const bool b1 = b >= 1 && b <= nb;
  switch (which) {
    case SRMI_FTRACE_LO:
      return b1 ? base + lo * (size_t)(b - 1) : (size_t)-1;
    case SRMI_FTRACE_PPOOL:
      return b1 ? base + lo * (size_t)nb + pp * (size_t)(b - 1) : (size_t)-1;
    case SRMI_FTRACE_RF:
      return b == 0 ? base + (lo + pp) * (size_t)nb : (size_t)-1;
    case SRMI_FTRACE_HB:
      return !e->train && b >= 0 && b <= nb ? inf + hbb * (size_t)b : (size_t)-1;
    case SRMI_FTRACE_T:
      return !e->train && b1 ? inf + hbb * (size_t)(nb + 1) + tb * (size_t)(b - 1) : (size_t)-1;
    case SRMI_FTRACE_REC:
      return !e->train && b1 ? inf + hbb * (size_t)(nb + 1) + tb * (size_t)nb + rc * (size_t)(b - 1) : (size_t)-1;
    default:
      return (size_t)-1;
  }
}
// one async device-to-device copy of the first n images' share of src into the slot
static int ftrace_copy(const srmi_engine* e, int which, int g, int b, const void* src, int n, hipStream_t st) {
  const size_t off = ftrace_offset(e, which, g, b);
  if (off == (size_t)-1) return SRMI_ERR_ARG;
  const hipError_t err =
      hipMemcpyAsync(e->ftrace + off, src, ftrace_piece_bytes(e, which, n), hipMemcpyDeviceToDevice, st);
  return err == hipSuccess ? 0 : -(int)err;
}
// the copies behind RCAB (g, b)'s last launch: the pair's lo8 bytes, and what an inference
// engine's rotating slots hold of this RCAB (pool: the strip records too, where that launch or
// the one before it wrote them and no launch between has its own copy site)
static int ftrace_rcab(const srmi_engine* e, int g, int b, bool pool, int n, hipStream_t st) {
  int rc = ftrace_copy(e, SRMI_FTRACE_LO, g, b, e->Hf, n, st);
  if (!rc && pool) rc = ftrace_copy(e, SRMI_FTRACE_PPOOL, g, b, e->ppool, n, st);
  if (!rc && !e->train) rc = ftrace_copy(e, SRMI_FTRACE_HB, g, b, e->hb(g, b), n, st);
  if (!rc && !e->train) rc = ftrace_copy(e, SRMI_FTRACE_T, g, b, e->Tm(g, b), n, st);
  if (!rc && !e->train) rc = ftrace_copy(e, SRMI_FTRACE_REC, g, b, e->recp(g, b), n, st);
  return rc;
}

// SRMI_TRACE_ERRORS=1 in the environment: every failing step prints its line
static int trace_rc(int rc, int line) {
  static const bool on = std::getenv("SRMI_TRACE_ERRORS") != nullptr;
  if (on) std::fprintf(stderr, "srmi: engine.cpp:%d -> %d\n", line, rc);
  return rc;
}
#define RC(x)                                  \
  do {                                         \
    int _rc = (x);                             \
    if (_rc) return trace_rc(_rc, __LINE__);   \
  } while (0)
#define HC(x)                                  \
  do {                                         \
    const hipError_t _he = (x);                \
    if (_he != hipSuccess) return -(int)_he;   \
  } while (0)

static int upload_tables(srmi_engine* e, hipStream_t st) {
  if (e->tables_uploaded) return 0;
  build_tables(e);
  hipError_t err = hipMemcpyAsync(e->d_entries, e->h_entries.data(), e->h_entries.size() * sizeof(PackEntry),
                                  hipMemcpyHostToDevice, st);
  if (err != hipSuccess) return -(int)err;
  if (!e->h_caoffs.empty()) {
    err = hipMemcpyAsync(e->d_caoffs, e->h_caoffs.data(), e->h_caoffs.size() * sizeof(long long),
                         hipMemcpyHostToDevice, st);
    if (err != hipSuccess) return -(int)err;
  }
  err = hipMemsetAsync(e->zeros, 0, 256, st);
  if (err != hipSuccess) return -(int)err;
  // the host vectors must outlive the async copies: keep them in the engine
  e->tables_uploaded = true;
  return 0;
}

// inference (no saved activations): each RCAB as one launch with a workgroup per image
// (rcab_infer.hip) -- bf16, 48-wide tiles, a CA bottleneck the MLP code handles
static bool use_rcab_infer(const srmi_engine* e) {
  const int CR = 64 / e->P.cfg.reduction;
  return !(e->P.cfg.flags & SRMI_FLAG_NO_RCAB_INFER) && !e->train && !e->f32 &&
         e->P.cfg.arch == SRMI_ARCH_RCAN && e->w == 48 && e->h % 4 == 0 && CR >= 4 && CR <= 32 && CR % 4 == 0;
}

// training forward: the CA forward of an RCAB (CALayer, sres/model/rcan/network.py:
// 31-47, 61-64) without a pass of its own.  conv1 writes t and its per-strip sums
// (EPI_RELU_POOL); conv2 (EPI_CA_RESID_U) stores u for backward and adds s bf16(u) into
// the residual pair in its epilogue, with s = the CA MLP of mean(u), and mean(u) from t's
// statistics and conv2's bf16 filter image (ca_scale.hpp), computed by every conv2
// workgroup in its prologue (its own launch between the convs measured -2.5 %).
// false: conv1, conv2 + pool writing u, the CA pass (ca_fwd) -- the exact-fp32 mode and tiles
// other than 48 wide always run this form; SRMI_FLAG_CA_PASS selects it at run time.
// true: bf16, 48-wide tiles, a bottleneck the scale code handles.
static bool ca_fwd_mode(const srmi_engine* e) {
  const int CR = 64 / e->P.cfg.reduction;
  return e->train && !e->f32 && e->P.cfg.arch == SRMI_ARCH_RCAN && e->w == 48 && e->h % 4 == 0 && CR >= 4 &&
         CR <= 32 && CR % 4 == 0 && !(e->P.cfg.flags & SRMI_FLAG_CA_PASS);
}

// ------------------------------------------------------------------ forward
static int forward_impl(srmi_engine* e, const float* prm, const float* lr, float* sr, int n, hipStream_t st) {
  const Plan& P = e->P;
  const int h = e->h, w = e->w, HW = h * w;
  const int nstrips = conv3x3_nstrips(h, w);
  RC(head_fwd_launch(lr, prm + P.head.w, prm + P.head.b, n, e->C, h, w, e->X0f, e->hb(0, 0), e->f32, st));
  if (e->ftrace && !e->train) RC(ftrace_copy(e, SRMI_FTRACE_HB, 0, 0, e->hb(0, 0), n, st));
  if (P.cfg.arch == SRMI_ARCH_RCAN) {
    const int nl = P.cfg.nlayers, nb = P.cfg.nblocks, R = P.cfg.reduction;
    for (int g = 0; g < nl; ++g) {
      const float* rin = g == 0 ? e->X0f : e->Rf;
      for (int b = 1; b <= nb; ++b) {
        const RCABRef& r = P.groups[g][b - 1];
        if (use_rcab_infer(e)) {  // inference: the RCAB as one launch, a workgroup per image
          uint8_t* lo = reinterpret_cast<uint8_t*>(e->Hf);  // the pair's lo8 remainder, 1 B / element
          const ConvParams c1 = fwd_params(e, r.c1, e->hb(g, b - 1), n, h, w, e->Tm(g, b), nullptr, nullptr, nullptr, 1.f);
          const ConvParams c2 = fwd_params(e, r.c2, e->Tm(g, b), n, h, w, e->Um(g, b), nullptr, nullptr, e->ppool, 1.f);
          RC(rcab_infer_launch(c1, c2, e->ppool, nstrips, prm + r.ca_w1, prm + r.ca_b1, prm + r.ca_w2, prm + r.ca_b2,
                               64 / R, b == 1 ? rin : nullptr, b == 1 ? nullptr : e->hb(g, b - 1),
                               b == 1 ? nullptr : lo, e->hb(g, b), lo, e->recp(g, b), st));
          if (e->ftrace) RC(ftrace_rcab(e, g, b, true, n, st));
          continue;
        }
        if (ca_fwd_mode(e)) {  // training: the CA forward inside conv2
          uint8_t* lo = reinterpret_cast<uint8_t*>(e->Hf);  // the pair's lo8 remainder (as below)
          ConvParams c1 = fwd_params(e, r.c1, e->hb(g, b - 1), n, h, w, e->Tm(g, b), nullptr, nullptr, e->ppool, 1.f);
          ConvParams c2 = fwd_params(e, r.c2, e->Tm(g, b), n, h, w, e->Um(g, b), nullptr, b == 1 ? rin : nullptr,
                                     nullptr, 1.f);
          // conv1's workgroups leave their share of the CA mean (the matvec on conv2's bf16
          // filter image) for conv2, which then reads no t border lines
          const int nruns = conv64_runs_per_image(c1);
          c1.cas.mpart = e->mpart;
          c1.cas.nruns = nruns;
          c1.cas.wimg = c2.w;
          c1.cas_on = 1;
          RC(conv3x3_launch(c1, EPI_RELU_POOL, st));
          if (e->ftrace) RC(ftrace_copy(e, SRMI_FTRACE_PPOOL, g, b, e->ppool, n, st));
          c2.r1h = b == 1 ? nullptr : e->hb(g, b - 1);
          c2.r1l = b == 1 ? nullptr : lo;
          c2.yph = e->hb(g, b);
          c2.ypl = lo;
          const CaScale cas{e->Tm(g, b), e->ppool, nstrips, prm + r.ca_w1, prm + r.ca_b1, prm + r.ca_w2,
                            prm + r.ca_b2, e->pbias + r.c2.pb_off, 64 / R, e->recp(g, b)};
          c2.cas = cas;
          c2.cas.mpart = e->mpart;
          c2.cas.nruns = nruns;
          c2.cas_on = 1;
          RC(conv3x3_launch(c2, EPI_CA_RESID_U, st));
          if (e->ftrace) RC(ftrace_rcab(e, g, b, false, n, st));
          continue;
        }
        RC(conv_fwd(e, r.c1, e->hb(g, b - 1), n, h, w, EPI_RELU_BF16, e->Tm(g, b), nullptr, nullptr, nullptr, 1.f, st));
        RC(conv_fwd(e, r.c2, e->Tm(g, b), n, h, w, EPI_POOL_BF16, e->Um(g, b), nullptr, nullptr, e->ppool, 1.f, st));
        if (e->f32) {
          RC(ca_fwd_launch(e->Um(g, b), e->ppool, nstrips, prm + r.ca_w1, prm + r.ca_b1, prm + r.ca_w2, prm + r.ca_b2,
                           n, HW, 64, R, b == 1 ? rin : e->Hf, e->Hf, e->hb(g, b), e->recp(g, b), 1, st));
        } else {
          // the residual stream inside the group as the pair hb (bf16, the next conv's
          // input) + lo (the 8-bit lo8 remainder, 1 B per element, in Hf's memory):
          // 16 significant bits per element (common.hpp); the group input rin is fp32
          uint8_t* lo = reinterpret_cast<uint8_t*>(e->Hf);
          RC(ca_fwd_launch(e->Um(g, b), e->ppool, nstrips, prm + r.ca_w1, prm + r.ca_b1, prm + r.ca_w2, prm + r.ca_b2,
                           n, HW, 64, R, b == 1 ? rin : nullptr, nullptr, e->hb(g, b), e->recp(g, b), 0, st,
                           b == 1 ? nullptr : e->hb(g, b - 1), b == 1 ? nullptr : lo, lo));
          if (e->ftrace) RC(ftrace_rcab(e, g, b, true, n, st));
        }
      }
      RC(conv_fwd(e, P.group_tail[g], e->hb(g, nb), n, h, w, EPI_RESID, e->hb(g + 1, 0), e->Rf, rin, nullptr, 1.f,
                  st));
      if (e->ftrace) {
        RC(ftrace_copy(e, SRMI_FTRACE_RF, g, 0, e->Rf, n, st));
        if (!e->train) RC(ftrace_copy(e, SRMI_FTRACE_HB, g + 1, 0, e->hb(g + 1, 0), n, st));
      }
    }
    RC(conv_fwd(e, P.body_tail, e->hb(nl, 0), n, h, w, EPI_RESID, e->RESb, nullptr, e->X0f, nullptr, 1.f, st));
  } else {
    const int nl = P.cfg.nlayers;
    for (int i = 0; i < nl; ++i) {
      const float* rin = i == 0 ? e->X0f : e->Rf;
      RC(conv_fwd(e, P.res1[i], e->hb(i, 0), n, h, w, EPI_RELU_BF16, e->Tm(i, 1), nullptr, nullptr, nullptr, 1.f, st));
      RC(conv_fwd(e, P.res2[i], e->Tm(i, 1), n, h, w, EPI_RESID, e->hb(i + 1, 0), e->Rf, rin, nullptr,
                  P.cfg.res_scale, st));
    }
    RC(conv_fwd(e, P.body_tail, e->hb(nl, 0), n, h, w, EPI_RESID, e->RESb, nullptr, e->X0f, nullptr, 1.f, st));
  }
  const bf16_t* cur = e->RESb;
  int H = h, W = w;
  for (int k = 0; k < P.nups; ++k) {
    RC(conv_fwd(e, P.ups[k], cur, n, H, W, EPI_PS_BF16, e->PS[k], nullptr, nullptr, nullptr, 1.f, st));
    cur = e->PS[k];
    H *= 2;
    W *= 2;
  }
  RC(tail_fwd_launch(cur, prm + P.tail.w, prm + P.tail.b, n, e->Co, H, W, sr, e->f32, st));
  e->last_n = n;
  e->next_stage = 0;
  if (!e->train) e->probe_prm = prm;  // (srmi_engine_probe which = 3)
  return 0;
}

// ----------------------------------------------------------------- backward
// Stages of the RCAN backward, in order: 0 = tail conv, upsamplers and body tail;
// 1 .. nlayers = residual groups nlayers-1 .. 0; nlayers + 1 = the head.  backward_impl
// runs stages s_lo .. s_hi (EDSR: all of them at once), so that a caller can enqueue a
// group's gradient all-reduce right behind that group (srmi_backward_stages).
static int backward_stages(const srmi_engine* e) { return e->P.cfg.arch == SRMI_ARCH_RCAN ? e->P.cfg.nlayers + 2 : 1; }

// The CALayer backward inside the fused conv2 backward (ca_bwd.hpp; SRMI_FLAG_DU_PASS off):
// the bf16 engine, a fusable 48-wide launch, CR = 64 / reduction in 4 .. 32 and a multiple
// of 4 (the MLP's thread mapping).  Else the CA backward is a launch of its own.
static bool du_in_f2(const srmi_engine* e, const ConvParams& cp, const WgradParams& wp, int epi) {
  const int CR = 64 / e->P.cfg.reduction;
  return !e->f32 && !(e->P.cfg.flags & SRMI_FLAG_DU_PASS) && epi == EPI_DG_RELUMASK &&
         rcab_bwd_fusable(cp, wp) && CR % 4 == 0 && CR >= 4 && CR <= 32;
}

static int backward_impl(srmi_engine* e, const float* prm, const float* lr, const float* sr, const float* hr,
                         const float* loss4, const float* dy, float* grads, void** group_events, hipStream_t st,
                         int s_lo = 0, int s_hi = 1 << 30) {
  const Plan& P = e->P;
  const int n = e->last_n, h = e->h, w = e->w, HW = h * w;
  const int nstrips = conv3x3_nstrips(h, w);
  int H = h << P.nups, W = w << P.nups;
  e->probe_prm = prm;
  const bool rcan = P.cfg.arch == SRMI_ARCH_RCAN;
  if (!rcan) {
    s_lo = 0;
    s_hi = 1 << 30;
  }
  const int nl = P.cfg.nlayers;
  if (s_lo <= 0) {
    // tail conv 64 -> C
    const bf16_t* xlast = e->PS[P.nups - 1];
    const float* yv = dy ? dy : sr;
    const float* tv = dy ? nullptr : hr;
    const float* lv = dy ? nullptr : loss4;
    RC(tail_dgrad_launch(yv, tv, lv, prm + P.tail.w, n, e->Co, H, W, e->dPS[P.nups - 1], e->f32, st));
    int nsl = 0;
    RC(tail_wgrad_launch(yv, tv, lv, xlast, n, e->Co, H, W, e->slab, &nsl, e->f32, st));
    RC(tail_wgrad_reduce_launch(e->slab, nsl, e->Co, grads + P.tail.w, grads + P.tail.b, st));
    // upsamplers, last to first
    for (int k = P.nups - 1; k >= 0; --k) {
      H /= 2;
      W /= 2;
      const bf16_t* xin = k == 0 ? e->RESb : e->PS[k - 1];
      RC(conv_wgrad(e, P.ups[k], xin, e->dPS[k], n, H, W, grads, true, 1.f, st));
      if (k > 0)
        RC(conv_dgrad(e, P.ups[k], e->dPS[k], n, H, W, EPI_PLAIN_BF16, e->dPS[k - 1], nullptr, nullptr, nullptr,
                      nullptr, nullptr, nullptr, 1.f, st));
      else
        RC(conv_dgrad(e, P.ups[k], e->dPS[k], n, H, W, EPI_DG_ACC, e->dRESb, e->dRESf, nullptr, nullptr, nullptr,
                      nullptr, nullptr, 1.f, st));
    }
  }
  // body tail: res = conv(hb_last) + x0
  float *gRf = e->GAf, *ghf = e->GBf;
  bf16_t *gRb = e->GAb, *ghb = e->GBb;
  if (rcan) {
    const int nb = P.cfg.nblocks, R = P.cfg.reduction;
    if (s_lo <= 0) {
      RC(conv_wgrad(e, P.body_tail, e->hb(nl, 0), e->dRESb, n, h, w, grads, true, 1.f, st));
      RC(conv_dgrad(e, P.body_tail, e->dRESb, n, h, w, EPI_DG_ACC, gRb, gRf, nullptr, nullptr, nullptr, nullptr,
                    nullptr, 1.f, st));
    }
    // One stream, two launches per RCAB:
    //   [the CA backward (MLP, du from g in LDS) -> dgrad conv2 -> dz || filter gradient conv2 (t, du)]
    //   [dgrad conv1 -> g (+ CA sums of the next RCAB)  ||  filter gradient conv1 (hb, dz)]
    // (SRMI_FLAG_DU_PASS, exact fp32, unfusable shapes: a CA-backward launch writing du
    // first).  The filter gradients write their RCAB's slab sets, reduced by one launch at
    // the group's end, before the group's event.
    const int rs2 = rcab_row_splits(e, n, 2), rs1 = rcab_row_splits(e, n, 1);
    // the gradient stream INSIDE a residual group (w.r.t. every RCAB output): bf16 in the
    // bf16 engine, in the buffer of the group input gradient's bf16 copy (ghb: the group's
    // first RCAB reads it and overwrites it in place with that copy), fp32 (ghf) in the
    // exact-fp32 engine.  The group input gradient itself stays fp32.
    const bool g16 = !e->f32;
    for (int g = nl - 1; g >= 0; --g) {
      const int stage = nl - g;
      // the gradient streams swap after every group: the state group g starts from
      const bool sw = ((nl - 1 - g) & 1) != 0;
      gRf = sw ? e->GBf : e->GAf;
      ghf = sw ? e->GAf : e->GBf;
      gRb = sw ? e->GBb : e->GAb;
      ghb = sw ? e->GAb : e->GBb;
      if (stage < s_lo || stage > s_hi) continue;
      const ConvRef& gt = P.group_tail[g];
      // (srmi_engine_trace: the in-group stream in the engine's operand type)
      const void* gstream = g16 ? static_cast<const void*>(ghb) : ghf;
      if (e->trace) RC(trace_copy(e, SRMI_TRACE_GRB, g, 0, gRb, n, st));
      // the filter-gradient reductions: collected for one launch at the group's end
      std::vector<ReduceSet> group_sets;
      // group tail: its dgrad (the bf16 stream's start, with the CA sums of RCAB nb) and its
      // filter gradient as one fused launch, like the RCABs' (slab set (0, 0), reduced with the
      // RCABs'), else (exact fp32, unfusable shapes) the two launches and the reduction in turn
      {
        int epi = EPI_DG_ACC;
        const ConvParams cp = dgrad_params(e, gt, gRb, n, h, w, &epi, g16 ? ghb : nullptr, g16 ? nullptr : ghf,
                                           nullptr, nullptr, nullptr, e->Um(g, nb), e->pacc, 1.f);
        WgradParams wp{};
        ReduceSet red{};
        if (g16)
          RC(wgrad_params(e, gt, e->hb(g, nb), gRb, n, h, w, grads, true, 1.f, rs1, e->slab_r(0, 0),
                          e->bslab_r(0, 0), e->slab_r_floats, e->bslab_r_floats, &wp, &red));
        if (g16 && rcab_bwd_fusable(cp, wp)) {
          RC(dgrad_with_wgrad(e, cp, epi, wp, 1, st));
          group_sets.push_back(red);
        } else {
          RC(conv_wgrad(e, gt, e->hb(g, nb), gRb, n, h, w, grads, true, 1.f, st));
          RC(conv3x3_launch(cp, epi, st));
        }
      }
      if (e->trace) {
        RC(trace_copy(e, SRMI_TRACE_STREAM, g, nb, gstream, n, st));
        RC(trace_copy(e, SRMI_TRACE_PACC, g, nb, e->pacc, n, st));
      }
      for (int b = nb; b >= 1; --b) {
        const RCABRef& r = P.groups[g][b - 1];
        bf16_t* du = e->DU;
        bf16_t* dz = e->DZ;
        ReduceSet red2, red1;
        WgradParams wp;
        int epi = EPI_DG_RELUMASK;
        ConvParams cp = dgrad_params(e, r.c2, du, n, h, w, &epi, dz, nullptr, nullptr, nullptr, nullptr, e->Tm(g, b),
                                     nullptr, 1.f);
        RC(wgrad_params(e, r.c2, e->Tm(g, b), du, n, h, w, grads, false, 1.f, rs2, e->slab_r(b, 0), e->bslab_r(b, 0),
                        e->slab_r_floats, e->bslab_r_floats, &wp, &red2, true));
        // The CALayer backward inside the fused conv2 backward (both its roles run the
        // image's MLP in their prologue and form du = bf16(g s + dm / HW) from the bf16
        // stream on their input rings; ca_bwd.hpp), or as a launch of its own writing du
        // (SRMI_FLAG_DU_PASS, exact fp32, unfusable shapes) that the conv2 backward reads
        const bool du_fused = du_in_f2(e, cp, wp, epi);
        if (du_fused) {
          cp.x = wp.dy = ghb;
          cp.gx = wp.gx = CaBwdIn{e->pacc, nstrips, e->recp(g, b), prm + r.ca_w1, prm + r.ca_w2, 64 / R,
                                  e->brecp(g, b), n, 1.f / (float)HW, 1};
        } else {
          RC(ca_bwd_du_launch(g16 ? static_cast<const void*>(ghb) : ghf, g16, e->pacc, nstrips, e->recp(g, b),
                              prm + r.ca_w1, prm + r.ca_w2, n, HW, 64, R, du, e->brecp(g, b), e->f32, st));
        }
        RC(dgrad_with_wgrad(e, cp, epi, wp, 2, st));
        if (e->trace) {
          RC(trace_copy(e, SRMI_TRACE_DZ, g, b, dz, n, st));
          if (!du_fused) RC(trace_copy(e, SRMI_TRACE_DU, g, b, du, n, st));
        }
        const bool last = (b == 1);
        epi = EPI_DG_ACC;
        // g += dgrad(dz): in the group's first RCAB into the group input gradient (fp32 +
        // its bf16 copy, with the group's skip gradient gR), else the in-group stream
        if (g16)
          cp = dgrad_params(e, r.c1, dz, n, h, w, &epi, ghb, last ? ghf : nullptr, nullptr, last ? gRf : nullptr,
                            (last && g == 0) ? e->dRESf : nullptr, last ? nullptr : e->Um(g, b - 1),
                            last ? nullptr : e->pacc, 1.f, ghb);
        else
          cp = dgrad_params(e, r.c1, dz, n, h, w, &epi, last ? ghb : nullptr, ghf, ghf, last ? gRf : nullptr,
                            (last && g == 0) ? e->dRESf : nullptr, last ? nullptr : e->Um(g, b - 1),
                            last ? nullptr : e->pacc, 1.f);
        RC(wgrad_params(e, r.c1, e->hb(g, b - 1), dz, n, h, w, grads, true, 1.f, rs1, e->slab_r(b, 1),
                        e->bslab_r(b, 1), e->slab_r_floats, e->bslab_r_floats, &wp, &red1, true));
        RC(dgrad_with_wgrad(e, cp, epi, wp, 1, st));
        if (e->trace) {
          RC(trace_copy(e, SRMI_TRACE_STREAM, g, b - 1, gstream, n, st));
          if (!last) RC(trace_copy(e, SRMI_TRACE_PACC, g, b - 1, e->pacc, n, st));
        }
        group_sets.push_back(red2);
        group_sets.push_back(red1);
      }
      if (!group_sets.empty()) RC(wgrad_reduce_sets_launch(group_sets.data(), (int)group_sets.size(), st));
      // per-RCAB slots of recp / brecp (N x 160 and N x 224 floats at any CR <= 32)
      RC(ca_param_grads_batched_launch(e->recp(g, 1), e->brecp(g, 1), nb, n, (size_t)e->N * 160, (size_t)e->N * 224,
                                       64, R, e->d_caoffs + (size_t)g * nb * 5, grads, st));
      // the group's gradients are final here (one stream): the hook for a bucketed
      // all-reduce overlapped with the rest of backward
      if (group_events && group_events[g]) HC(hipEventRecord(reinterpret_cast<hipEvent_t>(group_events[g]), st));
    }
    // after all nl groups: the group-0 input gradient (the head's upstream)
    gRf = (nl & 1) ? e->GBf : e->GAf;
  } else {
    const float rsc = P.cfg.res_scale;
    RC(conv_wgrad(e, P.body_tail, e->hb(nl, 0), e->dRESb, n, h, w, grads, true, 1.f, st));
    RC(conv_dgrad(e, P.body_tail, e->dRESb, n, h, w, EPI_DG_ACC, gRb, gRf, nullptr, nullptr, nullptr, nullptr, nullptr,
                  1.f, st));
    for (int i = nl - 1; i >= 0; --i) {
      // block i: out = rsc * (conv2(relu(conv1(x)))) + x, grad wrt out = gR
      RC(conv_wgrad(e, P.res2[i], e->Tm(i, 1), gRb, n, h, w, grads, true, rsc, st));
      RC(conv_dgrad(e, P.res2[i], gRb, n, h, w, EPI_DG_RELUMASK, e->DZ, nullptr, nullptr, nullptr, nullptr,
                    e->Tm(i, 1), nullptr, rsc, st));
      RC(conv_wgrad(e, P.res1[i], e->hb(i, 0), e->DZ, n, h, w, grads, true, 1.f, st));
      RC(conv_dgrad(e, P.res1[i], e->DZ, n, h, w, EPI_DG_ACC, ghb, ghf, gRf, i == 0 ? e->dRESf : nullptr, nullptr,
                    nullptr, nullptr, 1.f, st));
      std::swap(gRf, ghf);
      std::swap(gRb, ghb);
    }
  }
  // head: only the weight gradient (the input gradient is never read)
  if (s_hi >= (rcan ? nl + 1 : 0)) {
    int nsl = 0;
    RC(head_wgrad_launch(lr, gRf, n, e->C, h, w, e->slab, &nsl, st));
    RC(head_wgrad_reduce_launch(e->slab, nsl, e->C, grads + P.head.w, grads + P.head.b, st));
  }
  return 0;
}

// =================================================================== C ABI
extern "C" {

int srmi_version(void) { return 200; }

int srmi_param_count(const srmi_model_config* cfg, long long* n_params, int* n_tensors) {
  Plan P;
  RC(build_plan(cfg, P));
  if (n_params) *n_params = P.n_params;
  if (n_tensors) *n_tensors = (int)P.params.size();
  return 0;
}

int srmi_param_table(const srmi_model_config* cfg, srmi_param_info* out, int cap) {
  Plan P;
  RC(build_plan(cfg, P));
  if (!out || cap < (int)P.params.size()) return SRMI_ERR_ARG;
  std::memcpy(out, P.params.data(), P.params.size() * sizeof(srmi_param_info));
  return (int)P.params.size();
}

int srmi_workspace_size(const srmi_model_config* cfg, int train, size_t* bytes) {
  srmi_engine e;
  RC(init_engine(&e, cfg, train));
  *bytes = carve(&e, nullptr);
  return 0;
}

int srmi_engine_create(const srmi_model_config* cfg, void* workspace, size_t ws_bytes, int train, srmi_engine** out) {
  if (!out || !workspace) return SRMI_ERR_ARG;
  srmi_engine* e = new (std::nothrow) srmi_engine();
  if (!e) return SRMI_ERR_ARG;
  int rc = init_engine(e, cfg, train);
  if (rc) {
    delete e;
    return rc;
  }
  const size_t need = carve(e, nullptr);
  if (ws_bytes < need) {
    delete e;
    return SRMI_ERR_WORKSPACE;
  }
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  if ((size_t)(base - (char*)workspace) + need - 256 > ws_bytes) {
    delete e;
    return SRMI_ERR_WORKSPACE;
  }
  carve(e, base);
  *out = e;
  return 0;
}

int srmi_engine_destroy(srmi_engine* e) {
  delete e;
  return 0;
}

int srmi_pack_weights(srmi_engine* e, const float* params, void* stream) {
  if (!e || !params) return SRMI_ERR_ARG;
  RC(upload_tables(e, S_(stream)));
  return pack_launch(params, e->d_entries, (int)e->h_entries.size(), e->max_cob, e->max_cib, e->packs, e->pbias,
                     e->f32, S_(stream));
}

int srmi_forward(srmi_engine* e, const float* params, const float* lr, float* sr, int n, void* stream) {
  if (!e || !params || !lr || !sr || n < 1 || n > e->N) return SRMI_ERR_ARG;
  if (!e->tables_uploaded) return SRMI_ERR_ARG;  // srmi_pack_weights first
  return forward_impl(e, params, lr, sr, n, S_(stream));
}

int srmi_backward(srmi_engine* e, const float* params, const float* lr, const float* sr, const float* hr,
                  const float* loss4, const float* dy, float* grads, void** group_events, void* stream) {
  if (!e || !e->train || !params || !lr || !grads || e->last_n < 1) return SRMI_ERR_ARG;
  if (!dy && (!sr || !hr || !loss4)) return SRMI_ERR_ARG;
  if (e->next_stage != 0) return SRMI_ERR_ARG;  // a staged backward is half-way through
  return backward_impl(e, params, lr, sr, hr, loss4, dy, grads, group_events, S_(stream));
}

int srmi_backward_stage_count(srmi_engine* e) { return e ? backward_stages(e) : SRMI_ERR_ARG; }

int srmi_backward_stages(srmi_engine* e, const float* params, const float* lr, const float* sr, const float* hr,
                         const float* loss4, const float* dy, float* grads, void** group_events, int first, int last,
                         void* stream) {
  if (!e || !e->train || !params || !lr || !grads || e->last_n < 1) return SRMI_ERR_ARG;
  if (!dy && (!sr || !hr || !loss4)) return SRMI_ERR_ARG;
  const int ns = backward_stages(e);
  if (first < 0 || last >= ns || first > last || (ns == 1 && (first != 0 || last != 0))) return SRMI_ERR_ARG;
  if (first != e->next_stage) return SRMI_ERR_ARG;  // stages run in order, each once per backward
  RC(backward_impl(e, params, lr, sr, hr, loss4, dy, grads, group_events, S_(stream), first, last));
  e->next_stage = last + 1 == ns ? 0 : last + 1;
  return 0;
}

int srmi_engine_probe(srmi_engine* e, int which, int reps, void* stream) {
  if (which == 3) {  // inference engines: the one-launch RCAB (0, 2) of the last forward
    if (!e || e->train || !use_rcab_infer(e) || e->last_n < 1 || reps < 1 || e->P.cfg.nblocks < 2)
      return SRMI_ERR_ARG;
    const int n = e->last_n, R = e->P.cfg.reduction;
    const RCABRef& r = e->P.groups[0][1];
    const float* prm = e->probe_prm;
    if (!prm) return SRMI_ERR_ARG;
    uint8_t* lo = reinterpret_cast<uint8_t*>(e->Hf);
    const ConvParams c1 = fwd_params(e, r.c1, e->hb(0, 1), n, e->h, e->w, e->Tm(0, 2), nullptr, nullptr, nullptr, 1.f);
    const ConvParams c2 = fwd_params(e, r.c2, e->Tm(0, 2), n, e->h, e->w, e->Um(0, 2), nullptr, nullptr, e->ppool, 1.f);
    for (int i = 0; i < reps; ++i)
      RC(rcab_infer_launch(c1, c2, e->ppool, conv3x3_nstrips(e->h, e->w), prm + r.ca_w1, prm + r.ca_b1,
                           prm + r.ca_w2, prm + r.ca_b2, 64 / R, nullptr, e->hb(0, 1), lo, e->hb(0, 2), lo,
                           e->recp(0, 2), S_(stream)));
    return 0;
  }
  if (which == 8) {  // how the forward runs an RCAB
    if (!e || e->P.cfg.arch != SRMI_ARCH_RCAN) return SRMI_ERR_ARG;
    return use_rcab_infer(e) ? 2 : ca_fwd_mode(e) ? 1 : 0;
  }
  if (which == 5 || which == 6) {  // the filter gradients' row chunks per image of F1 (5) / F2 (6)
    if (!e || !e->train || e->P.cfg.arch != SRMI_ARCH_RCAN || e->last_n < 1) return SRMI_ERR_ARG;
    return rcab_row_splits(e, e->last_n, which == 5 ? 1 : 2);
  }
  if (which == 4 || which == 7) {  // 4: does the backward form du inside the fused conv2 backward (1) or not (0)
    if (!e || !e->train || e->P.cfg.arch != SRMI_ARCH_RCAN || e->last_n < 1 || !e->probe_prm) return SRMI_ERR_ARG;
    const int n = e->last_n, b = e->P.cfg.nblocks >= 2 ? 2 : 1;
    const RCABRef& r = e->P.groups[0][b - 1];
    int epi = EPI_DG_RELUMASK;
    ConvParams cp = dgrad_params(e, r.c2, e->DU, n, e->h, e->w, &epi, e->DZ, nullptr, nullptr, nullptr, nullptr,
                                 e->Tm(0, b), nullptr, 1.f);
    WgradParams wp;
    ReduceSet red;
    RC(wgrad_params(e, r.c2, e->Tm(0, b), e->DU, n, e->h, e->w, e->slab, false, 1.f, rcab_row_splits(e, n, 2),
                    e->slab_r(b, 0), e->bslab_r(b, 0), e->slab_r_floats, e->bslab_r_floats, &wp, &red, true));
    if (which == 7)  // how the RCAB backward launches run: fused | bf16 partial slabs | du formed in F2
      return (rcab_bwd_fusable(cp, wp) ? 1 : 0) | (wp.slab16 ? 2 : 0) | (du_in_f2(e, cp, wp, epi) ? 4 : 0);
    return du_in_f2(e, cp, wp, epi) ? 1 : 0;
  }
  if (!e || !e->train || e->P.cfg.arch != SRMI_ARCH_RCAN || e->last_n < 1 || reps < 1) return SRMI_ERR_ARG;
  if (which != 1 && which != 2) return SRMI_ERR_ARG;
  const int n = e->last_n, h = e->h, w = e->w;
  const int b = e->P.cfg.nblocks >= 2 ? 2 : 1;
  const RCABRef& r = e->P.groups[0][b - 1];
  float* ghf = e->GBf;
  float* grads = e->slab;  // the reductions are not launched: any pointer
  WgradParams wp;
  ReduceSet red;
  ConvParams cp;
  int epi;
  if (which == 2) {
    epi = EPI_DG_RELUMASK;
    cp = dgrad_params(e, r.c2, e->DU, n, h, w, &epi, e->DZ, nullptr, nullptr, nullptr, nullptr, e->Tm(0, b), nullptr,
                      1.f);
    RC(wgrad_params(e, r.c2, e->Tm(0, b), e->DU, n, h, w, grads, false, 1.f, rcab_row_splits(e, n, 2),
                    e->slab_r(b, 0), e->bslab_r(b, 0), e->slab_r_floats, e->bslab_r_floats, &wp, &red, true));
    // (as backward_impl: the CA backward and du inside the fused launch; its record and dm
    //  go to brec, which the engine's next backward rewrites)
    if (e->probe_prm && du_in_f2(e, cp, wp, epi)) {
      cp.x = wp.dy = e->GBb;
      cp.gx = wp.gx = CaBwdIn{e->pacc, conv3x3_nstrips(h, w), e->recp(0, b), e->probe_prm + r.ca_w1,
                              e->probe_prm + r.ca_w2, 64 / e->P.cfg.reduction, e->brecp(0, b), n, 1.f / (float)(h * w),
                              1};
    }
  } else {
    const bool last = (b == 1);
    epi = EPI_DG_ACC;
    if (!e->f32)  // the bf16 in-group gradient stream, as backward_impl issues it
      cp = dgrad_params(e, r.c1, e->DZ, n, h, w, &epi, e->GBb, last ? ghf : nullptr, nullptr, last ? e->GAf : nullptr,
                        nullptr, last ? nullptr : e->Um(0, b - 1), last ? nullptr : e->pacc, 1.f, e->GBb);
    else
      cp = dgrad_params(e, r.c1, e->DZ, n, h, w, &epi, last ? e->GAb : nullptr, ghf, ghf, last ? e->GAf : nullptr,
                        nullptr, last ? nullptr : e->Um(0, b - 1), last ? nullptr : e->pacc, 1.f);
    RC(wgrad_params(e, r.c1, e->hb(0, b - 1), e->DZ, n, h, w, grads, true, 1.f, rcab_row_splits(e, n, 1),
                    e->slab_r(b, 1), e->bslab_r(b, 1), e->slab_r_floats, e->bslab_r_floats, &wp, &red, true));
  }
  for (int i = 0; i < reps; ++i) RC(dgrad_with_wgrad(e, cp, epi, wp, which, S_(stream)));
  return 0;
}

int srmi_engine_buffer(srmi_engine* e, int which, int g, int b, void** ptr, size_t* elems, int* elem_bytes) {
  if (!e || !ptr || !elems || !elem_bytes) return SRMI_ERR_ARG;
  const bool rcan = e->P.cfg.arch == SRMI_ARCH_RCAN;
  const int nl = e->P.cfg.nlayers, nb = e->nbe();
  void* p = nullptr;
  size_t n = e->mapn;
  int eb = (int)e->esz;
  switch (which) {
    case SRMI_BUF_X0F:
      p = e->X0f;
      eb = 4;
      break;
    case SRMI_BUF_HB:  // (inference engines rotate three slots: no per-block map)
      if (!e->train || g < 0 || g > nl || b < 0 || b > (rcan && g < nl ? nb : 0)) return SRMI_ERR_ARG;
      p = e->hb(g, b);
      break;
    case SRMI_BUF_T:
      if (!e->train || g < 0 || g >= nl || b < 1 || b > nb) return SRMI_ERR_ARG;
      p = e->Tm(g, b);
      break;
    case SRMI_BUF_U:
      if (!e->train || !rcan || g < 0 || g >= nl || b < 1 || b > nb) return SRMI_ERR_ARG;
      p = e->Um(g, b);
      break;
    case SRMI_BUF_REC:
    case SRMI_BUF_BREC:
      if (!e->train || !rcan || g < 0 || g >= nl || b < 1 || b > nb) return SRMI_ERR_ARG;
      p = which == SRMI_BUF_REC ? e->recp(g, b) : e->brecp(g, b);
      n = (size_t)e->N * (which == SRMI_BUF_REC ? 160 : 224);
      eb = 4;
      break;
    case SRMI_BUF_DU:  // (EDSR has no du)
      if (!e->train || !rcan) return SRMI_ERR_ARG;
      p = e->DU;
      break;
    case SRMI_BUF_DZ:
      if (!e->train) return SRMI_ERR_ARG;
      p = e->DZ;
      break;
    case SRMI_BUF_DRESF:
      if (!e->train) return SRMI_ERR_ARG;
      p = e->dRESf;
      eb = 4;
      break;
    case SRMI_BUF_GROUP_IN_GRAD:  // backward_impl's ghf of group g (its streams swap after every group)
      if (!e->train || !rcan || g < 0 || g >= nl) return SRMI_ERR_ARG;
      p = ((nl - 1 - g) & 1) ? e->GAf : e->GBf;
      eb = 4;
      break;
    case SRMI_BUF_RESB:  // (both persist after a forward, in inference engines too)
      p = e->RESb;
      break;
    case SRMI_BUF_PS:
      if (g < 0 || g >= e->P.nups) return SRMI_ERR_ARG;
      p = e->PS[g];
      n = e->mapn << (2 * (g + 1));
      break;
    case SRMI_BUF_DPS:
      if (!e->train || g < 0 || g >= e->P.nups) return SRMI_ERR_ARG;
      p = e->dPS[g];
      n = e->mapn << (2 * (g + 1));
      break;
    case SRMI_BUF_DRESB:
      if (!e->train) return SRMI_ERR_ARG;
      p = e->dRESb;
      break;
    case SRMI_BUF_BODY_GRAD:  // backward_impl's gRf / gRb as the body tail's dgrad writes them
      if (!e->train || b < 0 || b > 1) return SRMI_ERR_ARG;
      p = b ? static_cast<void*>(e->GAb) : e->GAf;
      if (!b) eb = 4;
      break;
    case SRMI_BUF_HEAD_GRAD:  // backward_impl's gRf at the head (after nlayers swaps, RCAN and EDSR alike)
      if (!e->train) return SRMI_ERR_ARG;
      p = (nl & 1) ? e->GBf : e->GAf;
      eb = 4;
      break;
    default:
      return SRMI_ERR_ARG;
  }
  if (!p) return SRMI_ERR_ARG;
  *ptr = p;
  *elems = n;
  *elem_bytes = eb;
  return 0;
}

int srmi_engine_trace_size(srmi_engine* e, size_t* bytes) {
  if (!e || !bytes || !e->train || e->P.cfg.arch != SRMI_ARCH_RCAN) return SRMI_ERR_ARG;
  *bytes = trace_bytes(e);
  return 0;
}

int srmi_engine_trace(srmi_engine* e, void* buf, size_t bytes) {
  if (!e || !e->train || e->P.cfg.arch != SRMI_ARCH_RCAN) return SRMI_ERR_ARG;
  if (e->next_stage != 0) return SRMI_ERR_ARG;  // not half-way through a staged backward
  if (buf && (bytes < trace_bytes(e) || ((uintptr_t)buf & 255))) return SRMI_ERR_WORKSPACE;
  e->trace = static_cast<char*>(buf);
  return 0;
}

int srmi_engine_trace_slot(srmi_engine* e, int which, int g, int b, size_t* offset, size_t* elems, int* elem_bytes) {
  if (!e || !offset || !elems || !elem_bytes || !e->train || e->P.cfg.arch != SRMI_ARCH_RCAN) return SRMI_ERR_ARG;
  const size_t off = trace_offset(e, which, g, b);
  if (off == (size_t)-1) return SRMI_ERR_ARG;
  *offset = off;
  *elems = which == SRMI_TRACE_PACC ? (size_t)e->N * conv3x3_nstrips(e->h, e->w) * 128 : e->mapn;
  *elem_bytes = which == SRMI_TRACE_PACC ? 4 : (int)e->esz;
  return 0;
}

int srmi_engine_fwd_trace_size(srmi_engine* e, size_t* bytes) {
  if (!ftrace_engine(e) || !bytes) return SRMI_ERR_ARG;
  *bytes = ftrace_bytes(e);
  return 0;
}

int srmi_engine_fwd_trace(srmi_engine* e, void* buf, size_t bytes) {
  if (!ftrace_engine(e)) return SRMI_ERR_ARG;
  if (buf && (bytes < ftrace_bytes(e) || ((uintptr_t)buf & 255))) return SRMI_ERR_WORKSPACE;
  e->ftrace = static_cast<char*>(buf);
  return 0;
}

int srmi_engine_fwd_trace_slot(srmi_engine* e, int which, int g, int b, size_t* offset, size_t* elems,
                               int* elem_bytes) {
  if (!ftrace_engine(e) || !offset || !elems || !elem_bytes) return SRMI_ERR_ARG;
  const size_t off = ftrace_offset(e, which, g, b);
  if (off == (size_t)-1) return SRMI_ERR_ARG;
  const int eb = which == SRMI_FTRACE_LO ? 1 : (which == SRMI_FTRACE_HB || which == SRMI_FTRACE_T) ? 2 : 4;
  *offset = off;
  *elems = ftrace_piece_bytes(e, which, e->N) / (size_t)eb;
  *elem_bytes = eb;
  return 0;
}

int srmi_rmse_partial(srmi_engine* e, const float* pred, const float* target, size_t n, double count_global,
                      float* loss4, void* stream) {
  if (!e || !pred || !target || !loss4) return SRMI_ERR_ARG;
  RC(sqerr_partial_launch(pred, target, n, e->lpart, e->lpart_n, S_(stream)));
  return sqerr_finish_launch(e->lpart, e->lpart_n, count_global, loss4, S_(stream));
}

int srmi_rmse_partial_masked(srmi_engine* e, const float* pred, const float* target, size_t n, float* loss4,
                             void* stream) {
  if (!e || !pred || !target || !loss4) return SRMI_ERR_ARG;
  // the engine's partial buffer (lpart_n floats, 256-byte aligned) as {S, count} doubles of lpart_n / 4 blocks
  return sqerr_masked_launch(pred, target, n, reinterpret_cast<double*>(e->lpart), e->lpart_n / 4, loss4, S_(stream));
}

int srmi_charbonnier_partial(srmi_engine* e, const float* pred, const float* target, size_t n, double count_global,
                             float eps, float* loss4, float* dy, void* stream) {
  if (!e || !pred || !target || (!loss4 && !dy) || count_global <= 0) return SRMI_ERR_ARG;
  RC(charb_partial_launch(pred, target, n, eps, count_global, dy, loss4 ? e->lpart : nullptr, e->lpart_n, S_(stream)));
  return loss4 ? sqerr_finish_launch(e->lpart, e->lpart_n, count_global, loss4, S_(stream)) : 0;
}

// ---------------------------------------------------------------- op level
int srmi_conv3x3(const void* x, const void* wpack, const float* bias, int N, int H, int W, int Cin, int Cout,
                 int in_unshuffle, int epi, void* yb, float* yf, const float* r1, const float* r2, const float* r3,
                 const void* aux, float* part, float alpha, int dtype, void* stream) {
  if (dtype != SRMI_DTYPE_BF16 && dtype != SRMI_DTYPE_F32) return SRMI_ERR_ARG;
  ConvParams p{};
  p.f32 = dtype == SRMI_DTYPE_F32;
  p.x = (const bf16_t*)x;
  p.w = (const bf16_t*)wpack;
  p.bias = bias;
  p.N = N;
  p.H = H;
  p.W = W;
  p.Cin = Cin;
  p.Cout = Cout;
  p.in_mode = in_unshuffle ? IN_UNSHUF : IN_PLAIN;
  p.yb = (bf16_t*)yb;
  p.yf = yf;
  p.r1 = r1;
  p.r2 = r2;
  p.r3 = r3;
  p.aux = (const bf16_t*)aux;
  p.part = part;
  p.part_stride = (epi == EPI_DG_ACC || epi == EPI_DG_ACC_CA) ? 128 : Cout;
  p.alpha = alpha;
  return conv3x3_launch(p, epi, S_(stream));
}

int srmi_conv3x3_nstrips(int H, int W) { return conv3x3_nstrips(H, W); }

int srmi_wgrad3x3(const void* x, const void* dy, int N, int H, int W, int Cout, int dy_unshuffle, int row_splits,
                  float* slab, size_t slab_bytes, int ps, float alpha, float* gw, float* gb, int dtype, void* stream) {
  if (dtype != SRMI_DTYPE_BF16 && dtype != SRMI_DTYPE_F32) return SRMI_ERR_ARG;
  WgradParams p{};
  p.f32 = dtype == SRMI_DTYPE_F32;
  p.x = (const bf16_t*)x;
  p.dy = (const bf16_t*)dy;
  p.N = N;
  p.H = H;
  p.W = W;
  p.Cout = Cout;
  p.dy_mode = dy_unshuffle ? IN_UNSHUF : IN_PLAIN;
  p.imgs_per_wg = 1;
  p.row_splits = row_splits > 0 ? row_splits : choose_row_splits(N, H, Cout);
  const size_t ns = (size_t)wgrad3x3_nslabs(p);
  const size_t need = ns * Cout * 577 * sizeof(float) + 256;
  if (slab_bytes < need) return SRMI_ERR_WORKSPACE;
  p.slab = slab;
  p.bslab = slab + ns * Cout * 576;
  RC(wgrad3x3_launch(p, S_(stream)));
  if (!gw && !gb) return 0;  // partial slabs only (profiling the MFMA kernel alone)
  return wgrad_reduce_launch(p.slab, p.bslab, (int)ns, Cout, ps, wgrad3x3_slab_layout(p), alpha, gw, gb, S_(stream));
}

int srmi_ca_forward(const void* u, const float* part, int nstrips, const float* w1, const float* b1, const float* w2,
                    const float* b2, int N, int HW, int C, int R, const float* h_in, float* h_out, void* hb_out,
                    float* rec, int dtype, void* stream) {
  if (dtype != SRMI_DTYPE_BF16 && dtype != SRMI_DTYPE_F32) return SRMI_ERR_ARG;
  return ca_fwd_launch(u, part, nstrips, w1, b1, w2, b2, N, HW, C, R, h_in, h_out, hb_out, rec,
                       dtype == SRMI_DTYPE_F32, S_(stream));
}

int srmi_ca_forward_pair(const void* u, const float* part, int nstrips, const float* w1, const float* b1,
                         const float* w2, const float* b2, int N, int HW, int C, int R, const float* h_in,
                         const void* hi_in, const void* lo_in, void* hi_out, void* lo_out, float* rec, void* stream) {
  if (!hi_out || !lo_out || (!h_in && (!hi_in || !lo_in))) return SRMI_ERR_ARG;
  return ca_fwd_launch(u, part, nstrips, w1, b1, w2, b2, N, HW, C, R, h_in, nullptr, hi_out, rec, 0, S_(stream),
                       h_in ? nullptr : hi_in, h_in ? nullptr : lo_in, lo_out);
}

int srmi_ca_backward(const float* g, const float* part, int nstrips, const float* rec, const float* w1,
                     const float* w2, int N, int HW, int C, int R, void* du, float* brec, int dtype, void* stream) {
  if (dtype != SRMI_DTYPE_BF16 && dtype != SRMI_DTYPE_F32) return SRMI_ERR_ARG;
  return ca_bwd_du_launch(g, 0, part, nstrips, rec, w1, w2, N, HW, C, R, du, brec, dtype == SRMI_DTYPE_F32,
                          S_(stream));
}

int srmi_head_forward(const float* lr, const float* w, const float* b, int N, int C, int H, int W, float* x0f,
                      void* x0b, int dtype, void* stream) {
  if (dtype != SRMI_DTYPE_BF16 && dtype != SRMI_DTYPE_F32) return SRMI_ERR_ARG;
  return head_fwd_launch(lr, w, b, N, C, H, W, x0f, x0b, dtype == SRMI_DTYPE_F32, S_(stream));
}

int srmi_tail_forward(const void* x, const float* w, const float* b, int N, int C, int H, int W, float* y, int dtype,
                      void* stream) {
  if (dtype != SRMI_DTYPE_BF16 && dtype != SRMI_DTYPE_F32) return SRMI_ERR_ARG;
  return tail_fwd_launch(x, w, b, N, C, H, W, y, dtype == SRMI_DTYPE_F32, S_(stream));
}

}  // extern "C"
