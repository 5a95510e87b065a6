// Proof of serl_amd/csrc/dense_layer.h on the CPU (tests/test_dense_layer_cpu.py builds this with the host address and
// undefined-behaviour sanitizers).  For each of the update chain's six Dense -> LayerNorm -> activation layers -- camera
// bottleneck, proprio branch, critic layers 1 and 2, policy layers 1 and 2 -- the description is built the way build_layout
// builds it, and the six argument structs derived from it (forward GEMM, LayerNorm forward, LayerNorm backward, column sums,
// kernel gradient, input gradient) are compared field by field with the explicit form: the row of positional arguments that
// agent.hip wrote at every call site before the layer was stated once, kept here in full.  Nothing is dereferenced; the pointers
// are places in one host arena.
//
// Two kinds of field have no explicit value to hold to, because no kernel reads them and the call sites themselves disagreed
// (the policy's forward wrote y_goff = rows * hidden, its backward 0): a group stride or offset of a struct with ONE group, which
// only group index 0 multiplies, and `beta` of a LayerNorm backward whose activation is not swish.  The description fills both
// like any other field; GS() and the beta check below accept exactly these and nothing else.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dense_layer.h"

using namespace serl;

static const char* g_case = "";
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s: %s (line %d)\n", g_case, #c, __LINE__); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)
#define GS(a, b, groups) CHECK((a) == (b) || (groups) == 1)   // a group stride / offset

static void same(const GemmDesc& a, const GemmDesc& b) {   // a: derived, b: explicit
  CHECK(a.A == b.A && a.B == b.B && a.C == b.C && a.M == b.M && a.N == b.N && a.K == b.K);
  CHECK(a.sAm == b.sAm && a.sAk == b.sAk && a.sBk == b.sBk && a.sBn == b.sBn && a.ldc == b.ldc);
  GS(a.sAb, b.sAb, b.nbatch);
  GS(a.sBb, b.sBb, b.nbatch);
  GS(a.sCz, b.sCz, b.nbatch * b.splitk);
  CHECK(a.nbatch == b.nbatch && a.splitk == b.splitk);
  CHECK(a.gtab == b.gtab && a.gseg == b.gseg && a.gkbias == b.gkbias && a.gpitch == b.gpitch && a.relu == b.relu);
  CHECK(a.epi == b.epi && a.ctr == b.ctr && a.zred == b.zred && a.out == b.out && a.ld_out == b.ld_out && a.out_gstride == b.out_gstride);
}
static void same(const LnFwdArgs& a, const LnFwdArgs& b) {
  const int groups = b.rows / b.rows_per_group;
  CHECK(a.slabs == b.slabs && a.S == b.S && a.slab_stride == b.slab_stride);
  CHECK(a.bias == b.bias && a.gamma == b.gamma && a.beta == b.beta);
  GS(a.pstride, b.pstride, groups);
  CHECK(a.rows == b.rows && a.rows_per_group == b.rows_per_group && a.y == b.y && a.ld_y == b.ld_y);
  GS(a.y_goff, b.y_goff, groups);
  CHECK(a.xhat == b.xhat && a.rstd == b.rstd && a.act == b.act);
  CHECK(a.dot_w == b.dot_w && a.dot_b == b.dot_b && a.dot_out == b.dot_out && a.dot_gstride == b.dot_gstride && a.dot_b_gstride == b.dot_b_gstride);
}
static void same(const LnBwdArgs& a, const LnBwdArgs& b, const float* beta) {   // beta: the layer's LayerNorm bias
  const int groups = b.rows / b.rows_per_group;
  CHECK(a.dy == b.dy && a.ld_dy == b.ld_dy && a.y == b.y && a.ld_y == b.ld_y);
  GS(a.dy_goff, b.dy_goff, groups);
  GS(a.y_goff, b.y_goff, groups);
  CHECK(a.dq == b.dq && a.dq_w == b.dq_w && a.dq_const == b.dq_const && a.dq_w_gstride == b.dq_w_gstride && a.dq_inline == b.dq_inline);
  CHECK(a.xhat == b.xhat && a.rstd == b.rstd && a.gamma == b.gamma);
  GS(a.pstride, b.pstride, groups);
  CHECK(a.rows == b.rows && a.rows_per_group == b.rows_per_group && a.D == b.D && a.dx == b.dx && a.dg == b.dg && a.act == b.act);
  CHECK(a.beta == beta && (b.beta == beta || (b.beta == nullptr && b.act != kActSwish)));
}
static void same(const Colsum3Args& a, const Colsum3Args& b) {
  CHECK(a.dg == b.dg && a.xhat == b.xhat && a.dpre == b.dpre && a.groups == b.groups && a.rows_per_group == b.rows_per_group && a.D == b.D);
  CHECK(a.o_gamma == b.o_gamma && a.o_beta == b.o_beta && a.o_bias == b.o_bias && a.mode == b.mode);
  GS(a.gstride, b.gstride, b.groups);
}

// the explicit LayerNorm forward / backward of the call sites: dense_ln_multi's and cam_dense_ln_args' body, ln_bwd_args + dense_ln_bwd's
static LnFwdArgs ln_fwd_explicit(float* slabs, int S, long slab_stride, const float* bias, const float* gamma, const float* beta,
                                 long pstride, int groups, int rows, float* y, long ld_y, long y_goff, float* xhat, float* rstd, int act) {
  LnFwdArgs l{};
  l.slabs = slabs; l.S = S; l.slab_stride = slab_stride;
  l.bias = bias; l.gamma = gamma; l.beta = beta; l.pstride = pstride;
  l.rows = groups * rows; l.rows_per_group = rows;
  l.y = y; l.ld_y = ld_y; l.y_goff = y_goff;
  l.xhat = xhat; l.rstd = rstd; l.act = act;
  return l;
}
static LnBwdArgs ln_bwd_explicit(const float* dy, long ld_dy, long dy_goff, const float* y, long ld_y, long y_goff, const float* xhat,
                                 const float* rstd, const float* gamma, const float* beta, int act, long p_gstride, int groups,
                                 int rows, int D, float* dpre, float* dg) {
  LnBwdArgs l{};
  l.dy = dy; l.ld_dy = ld_dy; l.dy_goff = dy_goff;
  l.y = y; l.ld_y = ld_y; l.y_goff = y_goff;
  l.xhat = xhat; l.rstd = rstd; l.gamma = gamma; l.pstride = p_gstride;
  l.rows = groups * rows; l.rows_per_group = rows; l.D = D;
  l.dx = dpre; l.dg = dg;
  l.act = act; l.beta = beta;
  return l;
}

struct Arena {   // distinct places for the tensors of a case
  std::vector<float> mem = std::vector<float>(1 << 16);
  size_t used = 0;
  float* take(size_t n = 64) { float* p = mem.data() + used; used += n; CHECK(used <= mem.size()); return p; }
};

// One agent shape: n_cam cameras, `ens` critics, `rows` rows of a batch of `batch`; widths as in the header of the test module.
static void run_case(int n_cam, int ens, int rows, int batch) {
  static char name[96];
  std::snprintf(name, sizeof name, "cams=%d ens=%d rows=%d batch=%d", n_cam, ens, rows, batch);
  g_case = name;
  const int D = 4096, Bn = 256, S = 19, Pd = 64, Hd = 128, A = 6, sle = 1000;
  const int E = n_cam * Bn + Pd, XA = E + A, cact = kActSwish, pact = kActRelu;
  // ---- the layout, as build_layout lays it out: cameras (an embedding kernel in front of each), critic, proprio, policy
  std::vector<Leaf> L;
  long off = 0;
  const CamHeadOffsets ch = add_cam_head_leaves(L, off, n_cam, D, Bn, [&](const std::string& p) { add_leaf(L, off, p + "sle", sle); });
  const DenseLn cam = ch.dense;
  const long cam_stride = n_cam > 1 ? find(L, "enc/1/sle")->off - find(L, "enc/0/sle")->off : off;   // (as the call sites had it)
  CHECK(ch.first == find(L, "enc/0/sle")->off && ch.stride == cam_stride && cam.groups == n_cam);
  const DenseLn c1 = add_dense_ln_leaves(L, off, "critic/w1", "critic/b1", "critic/ln1", ens, XA, Hd, cact);
  const DenseLn c2 = add_dense_ln_leaves(L, off, "critic/w2", "critic/b2", "critic/ln2", ens, Hd, Hd, cact);
  const DenseLn prop = add_dense_ln_leaves(L, off, "enc/proprio/dense/kernel", "enc/proprio/dense/bias", "enc/proprio/ln", 1, S, Pd, kActTanh);
  const DenseLn a1 = add_dense_ln_leaves(L, off, "actor/w1", "actor/b1", "actor/ln1", 1, E, Hd, pact);
  const DenseLn a2 = add_dense_ln_leaves(L, off, "actor/w2", "actor/b2", "actor/ln2", 1, Hd, Hd, pact);
  // ... and the same offsets under the names the call sites used
  const long dW = find(L, "enc/0/dense/kernel")->off, db = find(L, "enc/0/dense/bias")->off, lng = find(L, "enc/0/ln/scale")->off,
             lnb = find(L, "enc/0/ln/bias")->off;
  const long c_w1 = find(L, "critic/w1")->off, c_b1 = find(L, "critic/b1")->off, c_g1 = find(L, "critic/ln1/scale")->off, c_be1 = find(L, "critic/ln1/bias")->off;
  const long c_w2 = find(L, "critic/w2")->off, c_b2 = find(L, "critic/b2")->off, c_g2 = find(L, "critic/ln2/scale")->off, c_be2 = find(L, "critic/ln2/bias")->off;
  const long p_W = find(L, "enc/proprio/dense/kernel")->off, p_b = find(L, "enc/proprio/dense/bias")->off, p_g = find(L, "enc/proprio/ln/scale")->off,
             p_be = find(L, "enc/proprio/ln/bias")->off;
  const long a_w1 = find(L, "actor/w1")->off, a_b1 = find(L, "actor/b1")->off, a_g1 = find(L, "actor/ln1/scale")->off, a_be1 = find(L, "actor/ln1/bias")->off;
  const long a_w2 = find(L, "actor/w2")->off, a_b2 = find(L, "actor/b2")->off, a_g2 = find(L, "actor/ln2/scale")->off, a_be2 = find(L, "actor/ln2/bias")->off;
  CHECK(cam_stride == sle + (long)D * Bn + 3 * Bn);
  CHECK(c_b1 == c_w1 + (long)ens * XA * Hd && c_w2 == c_be1 + (long)ens * Hd && p_W == c_be2 + (long)ens * Hd && a_w1 == p_be + Pd);
  std::vector<float> Pv((size_t)off), Gv((size_t)off);
  const float* P = Pv.data();
  float* G = Gv.data();
  Arena ar;
  float* slabs = ar.take();
  const long N = ens;   // (the call sites' name for the ensemble size)
  const int cnt = rows;

  {   // ---- camera bottleneck: encode_multi (cam_dense_ln_args) and enc_bwd_critic; the output is a column slice of the code
    float *f = ar.take(), *enc = ar.take(), *xhat = ar.take(), *rstd = ar.take(), *dx = ar.take(), *dz = ar.take(), *dgz = ar.take(), *df = ar.take();
    const long ld = XA;   // (encO: the code is the front of the critic's input row)
    const DenseLnIo t{f, D, (long)batch * D, enc, ld, Bn, xhat, rstd};
    const DenseLnGrad d{dx, XA, Bn, dz, dgz};
    const int S0 = 32;
    const GemmDesc g = layer_fwd(cam, P, t, cnt, slabs, S0);
    same(g, gemm_fwd(f, D, (long)batch * D, P + dW, cam_stride, slabs, n_cam, cnt, Bn, D, S0));
    same(layer_ln_fwd(cam, P, t, cnt, g),
         ln_fwd_explicit(slabs, S0, (long)cnt * Bn, P + db, P + lng, P + lnb, cam_stride, n_cam, cnt, enc, ld, Bn, xhat, rstd, kActTanh));
    same(layer_ln_bwd(cam, P, t, d, cnt),
         ln_bwd_explicit(dx, XA, Bn, enc, ld, Bn, xhat, rstd, P + lng, nullptr, kActTanh, cam_stride, n_cam, cnt, Bn, dz, dgz), P + lnb);
    same(layer_colsum(cam, t, d, cnt, G), Colsum3Args{dgz, xhat, dz, n_cam, cnt, Bn, G + lng, G + lnb, G + db, cam_stride, 0});
    same(layer_wgrad(cam, t, d, cnt, G), gemm_wgrad(f, D, (long)batch * D, dz, Bn, (long)cnt * Bn, G + dW, Bn, cam_stride, n_cam, D, Bn, cnt));
    same(layer_igrad(cam, P, d, cnt, df, D, (long)cnt * D),
         gemm_igrad(dz, Bn, (long)cnt * Bn, P + dW, Bn, cam_stride, df, D, (long)cnt * D, n_cam, cnt, D, Bn));
  }
  {   // ---- proprio branch: proprio_bwd.  (Its forward is a row kernel and its input the state: the forward and input-gradient
      // GEMMs have no call site; they are held to the primitive forms of the same operands.)
    float *state = ar.take(), *enc = ar.take(2048), *pxhat = ar.take(), *prstd = ar.take(), *dy = ar.take(), *dp = ar.take(), *dgp = ar.take(), *ds = ar.take();
    const long pc = (long)n_cam * Bn, ld = E, ld_dy = Pd;
    const DenseLnIo t{state, S, 0, enc + pc, ld, 0, pxhat, prstd};
    const DenseLnGrad d{dy, ld_dy, 0, dp, dgp};
    const GemmDesc g = layer_fwd(prop, P, t, cnt, slabs, 1);
    same(g, gemm_fwd(state, S, 0, P + p_W, 0, slabs, 1, cnt, Pd, S, 1));
    same(layer_ln_fwd(prop, P, t, cnt, g),
         ln_fwd_explicit(slabs, 1, (long)cnt * Pd, P + p_b, P + p_g, P + p_be, 0, 1, cnt, enc + pc, ld, 0, pxhat, prstd, kActTanh));
    same(layer_ln_bwd(prop, P, t, d, cnt),
         ln_bwd_explicit(dy, ld_dy, 0, enc + pc, ld, 0, pxhat, prstd, P + p_g, nullptr, kActTanh, 0, 1, cnt, Pd, dp, dgp), P + p_be);
    same(layer_colsum(prop, t, d, cnt, G), Colsum3Args{dgp, pxhat, dp, 1, cnt, Pd, G + p_g, G + p_be, G + p_b, 0, 0});
    same(layer_wgrad(prop, t, d, cnt, G), gemm_wgrad(state, S, 0, dp, Pd, 0, G + p_W, Pd, 0, 1, S, Pd, cnt));
    same(layer_igrad(prop, P, d, cnt, ds, S, 0), gemm_igrad(dp, Pd, 0, P + p_W, Pd, 0, ds, S, 0, 1, cnt, S, Pd));
  }
  // the MLPs' tensors: critic_fwd_multi / critic_bwd, policy_fwd_multi / serl_agent_actor_grads
  float *x = ar.take(), *h1 = ar.take(), *xh1 = ar.take(), *rs1 = ar.take(), *h2 = ar.take(), *xh2 = ar.take(), *rs2 = ar.take();
  float *dh2 = ar.take(), *da2 = ar.take(), *dg2 = ar.take(), *dh1 = ar.take(), *da1 = ar.take(), *dg1 = ar.take(), *dxo = ar.take();
  {   // ---- critic layer 1: every member reads the one input x, and writes its block of h1
    const DenseLnIo t{x, XA, 0, h1, Hd, (long)cnt * Hd, xh1, rs1};
    const DenseLnGrad d{dh1, Hd, (long)cnt * Hd, da1, dg1};
    const GemmDesc g = layer_fwd(c1, P, t, cnt, slabs, 4);
    same(g, gemm_fwd(x, XA, 0, P + c_w1, (long)XA * Hd, slabs, N, cnt, Hd, XA, 4));
    same(layer_ln_fwd(c1, P, t, cnt, g),
         ln_fwd_explicit(slabs, 4, (long)cnt * Hd, P + c_b1, P + c_g1, P + c_be1, Hd, N, cnt, h1, Hd, (long)cnt * Hd, xh1, rs1, cact));
    same(layer_ln_bwd(c1, P, t, d, cnt),
         ln_bwd_explicit(dh1, Hd, (long)cnt * Hd, h1, Hd, (long)cnt * Hd, xh1, rs1, P + c_g1, P + c_be1, cact, Hd, N, cnt, Hd, da1, dg1), P + c_be1);
    same(layer_colsum(c1, t, d, cnt, G), Colsum3Args{dg1, xh1, da1, (int)N, cnt, Hd, G + c_g1, G + c_be1, G + c_b1, Hd, 0});
    same(layer_wgrad(c1, t, d, cnt, G), gemm_wgrad(x, XA, 0, da1, Hd, (long)cnt * Hd, G + c_w1, Hd, (long)XA * Hd, N, XA, Hd, cnt));
    // (igrad_sum gives this GEMM its slabs: the plain form of SERL_CHAIN_FUSE=0 here)
    same(layer_igrad(c1, P, d, cnt, slabs, XA, (long)cnt * XA),
         gemm_igrad(da1, Hd, (long)cnt * Hd, P + c_w1, Hd, (long)XA * Hd, slabs, XA, (long)cnt * XA, N, cnt, XA, Hd));
  }
  {   // ---- critic layer 2: every member on its block of h1; dy is formed in the launch (rank-1), the input gradient is layer 1's dy
    const DenseLnIo t{h1, Hd, (long)cnt * Hd, h2, Hd, (long)cnt * Hd, xh2, rs2};
    const DenseLnGrad d{nullptr, Hd, (long)cnt * Hd, da2, dg2}, below{dh1, Hd, (long)cnt * Hd, da1, dg1};
    const GemmDesc g = layer_fwd(c2, P, t, cnt, slabs, 2);
    same(g, gemm_fwd(h1, Hd, (long)cnt * Hd, P + c_w2, (long)Hd * Hd, slabs, N, cnt, Hd, Hd, 2));
    same(layer_ln_fwd(c2, P, t, cnt, g),
         ln_fwd_explicit(slabs, 2, (long)cnt * Hd, P + c_b2, P + c_g2, P + c_be2, Hd, N, cnt, h2, Hd, (long)cnt * Hd, xh2, rs2, cact));
    same(layer_ln_bwd(c2, P, t, d, cnt),
         ln_bwd_explicit(nullptr, Hd, (long)cnt * Hd, h2, Hd, (long)cnt * Hd, xh2, rs2, P + c_g2, P + c_be2, cact, Hd, N, cnt, Hd, da2, dg2), P + c_be2);
    same(layer_colsum(c2, t, d, cnt, G), Colsum3Args{dg2, xh2, da2, (int)N, cnt, Hd, G + c_g2, G + c_be2, G + c_b2, Hd, 0});
    same(layer_wgrad(c2, t, d, cnt, G), gemm_wgrad(h1, Hd, (long)cnt * Hd, da2, Hd, (long)cnt * Hd, G + c_w2, Hd, (long)Hd * Hd, N, Hd, Hd, cnt));
    same(layer_igrad(c2, P, d, cnt, below),
         gemm_igrad(da2, Hd, (long)cnt * Hd, P + c_w2, Hd, (long)Hd * Hd, dh1, Hd, (long)cnt * Hd, N, cnt, Hd, Hd));
  }
  {   // ---- policy layer 1 (one group): reads the code, a row of width E
    float* enc = ar.take();
    const DenseLnIo t{enc, E, 0, h1, Hd, (long)cnt * Hd, xh1, rs1};
    const DenseLnGrad d{dh1, Hd, (long)cnt * Hd, da1, dg1};
    const GemmDesc g = layer_fwd(a1, P, t, cnt, slabs, 8);
    same(g, gemm_fwd(enc, E, 0, P + a_w1, 0, slabs, 1, cnt, Hd, E, 8));
    same(layer_ln_fwd(a1, P, t, cnt, g),
         ln_fwd_explicit(slabs, 8, (long)cnt * Hd, P + a_b1, P + a_g1, P + a_be1, 0, 1, cnt, h1, Hd, (long)cnt * Hd, xh1, rs1, pact));
    same(layer_ln_bwd(a1, P, t, d, cnt),
         ln_bwd_explicit(dh1, Hd, 0, h1, Hd, 0, xh1, rs1, P + a_g1, P + a_be1, pact, 0, 1, cnt, Hd, da1, dg1), P + a_be1);
    same(layer_colsum(a1, t, d, cnt, G), Colsum3Args{dg1, xh1, da1, 1, cnt, Hd, G + a_g1, G + a_be1, G + a_b1, 0, 0});
    same(layer_wgrad(a1, t, d, cnt, G), gemm_wgrad(enc, E, 0, da1, Hd, 0, G + a_w1, Hd, 0, 1, E, Hd, cnt));
    same(layer_igrad(a1, P, d, cnt, dxo, E, 0), gemm_igrad(da1, Hd, 0, P + a_w1, Hd, 0, dxo, E, 0, 1, cnt, E, Hd));
  }
  {   // ---- policy layer 2
    const DenseLnIo t{h1, Hd, 0, h2, Hd, (long)cnt * Hd, xh2, rs2};
    const DenseLnGrad d{dh2, Hd, (long)cnt * Hd, da2, dg2}, below{dh1, Hd, (long)cnt * Hd, da1, dg1};
    const GemmDesc g = layer_fwd(a2, P, t, cnt, slabs, 4);
    same(g, gemm_fwd(h1, Hd, 0, P + a_w2, 0, slabs, 1, cnt, Hd, Hd, 4));
    same(layer_ln_fwd(a2, P, t, cnt, g),
         ln_fwd_explicit(slabs, 4, (long)cnt * Hd, P + a_b2, P + a_g2, P + a_be2, 0, 1, cnt, h2, Hd, (long)cnt * Hd, xh2, rs2, pact));
    same(layer_ln_bwd(a2, P, t, d, cnt),
         ln_bwd_explicit(dh2, Hd, 0, h2, Hd, 0, xh2, rs2, P + a_g2, P + a_be2, pact, 0, 1, cnt, Hd, da2, dg2), P + a_be2);
    same(layer_colsum(a2, t, d, cnt, G), Colsum3Args{dg2, xh2, da2, 1, cnt, Hd, G + a_g2, G + a_be2, G + a_b2, 0, 0});
    same(layer_wgrad(a2, t, d, cnt, G), gemm_wgrad(h1, Hd, 0, da2, Hd, 0, G + a_w2, Hd, 0, 1, Hd, Hd, cnt));
    same(layer_igrad(a2, P, d, cnt, below), gemm_igrad(da2, Hd, 0, P + a_w2, Hd, 0, dh1, Hd, 0, 1, cnt, Hd, Hd));
  }
  std::printf("case %s ok\n", name);
}

int main() {
  for (int n_cam : {1, 3})
    for (int ens : {2, 3})
      for (int rows : {1, 5, 65}) run_case(n_cam, ens, rows, rows == 5 ? 5 : 70);   // rows == batch, and a minibatch of a larger batch
  std::printf("ok\n");
  return 0;
}
