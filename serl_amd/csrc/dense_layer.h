// The Dense -> LayerNorm -> activation layer of the update chain, stated once (host only): camera bottleneck, proprio branch and
// the two layers of the critic and of the policy, each over `groups` parameter groups (cameras, ensemble members).  A layout
// describes the layer (DenseLn), a carve the tensors of one evaluation (DenseLnIo) and of one backward pass (DenseLnGrad); the
// functions below derive the arguments of every launch that touches the layer, so that no caller writes one of its strides.
// Fields that only group index 0 multiplies (one group) are filled like any other; `beta` is always passed (the swish backward reads it).
// A layer of an MLP with use_layer_norm=False (mlp.py:29-30) is the same layer without the LayerNorm ("plain", DenseLn::ln == 0):
// y = act(Dense(x) + b), two leaves, and the same launches one for one -- the row launches take its arguments without gamma and beta.
#pragma once
#include "heads.h"

namespace serl {

struct DenseLn {
  long W, b, g, be;      // group 0's kernel [K][N], bias, LayerNorm scale and LayerNorm bias: offsets into a parameter vector
  long w_gs, p_gs;       // floats from one group's kernel, and from one group's three vectors, to the next group's
  int groups, K, N, act; // act: kAct*
  int Nt;                // the layer's true width, Nt <= N.  Nt < N: a ragged layer stored N = 64 ceil(Nt / 64) wide, columns [Nt, N)
                         // of its kernel and vectors zero (and rows [Kt, K) of its kernel, where its input is ragged too)
  int ln;                // 1: LayerNorm between Dense and activation; 0: none (mlp.py:29-30) -- g and be are then -1, no leaves
  float keep;            // Dropout between Dense and LayerNorm (mlp.py:27-28): float32(1 - rate), the rate a double in (0, 1) as the
                         // reference's keep_prob = 1.0 - rate is one -- what its bernoulli compares with and its division divides by; 0: none
};
// Where the keep decisions of ONE evaluation (a "site") of a Dropout layer come from, in this order of preference:
struct DenseLnDrop {   // (of a layer with keep > 0)
  int train;               // 0: train=False, no Dropout in this evaluation (the zero-initialised site)
  const uint8_t* mask;     // a device keep-mask u8 [rows][N] of the evaluation's rows (one mask for every group), or
  const uint32_t* key;     // a host jax.random key: bernoulli(key, keep, (key_rows, N)), rows key_row0.., or
  uint64_t seed;           // the hash stream `seed`, indexed by the global row: local row 0 is row hash_row0
  long key_rows, key_row0, hash_row0;
};
// the layer's Dropout as the LayerNorm rows take it (forward and backward alike); a layer without Dropout ignores the site, and
// a train=False evaluation drops nothing
inline LnDrop layer_drop(const DenseLn& L, const DenseLnDrop& s) {
  LnDrop d{};
  if (!(L.keep > 0.f) || !s.train) return d;
  d.keep = L.keep;
  if (s.mask) { d.mode = kLnDropMask; d.mask = s.mask; }
  else if (s.key) { d.mode = kLnDropKey; d.key[0] = s.key[0]; d.key[1] = s.key[1]; d.total_rows = s.key_rows; d.row0 = s.key_row0; }
  else { d.mode = kLnDropHash; d.seed = s.seed; d.row0 = s.hash_row0; }
  return d;
}
// Appends the layer's four leaves -- `groups` kernels, biases, scales and shifts back to back in each -- at `off`, which moves
// behind them.  layer_norm false: the kernels and biases alone.  Kt / Nt (0: K / N): the true extents of a ragged layer, whose
// leaves are boxes [Kt][Nt] and [Nt] inside the storage [K][N] and [N] (param_arena.h).
inline DenseLn add_dense_ln_leaves(std::vector<Leaf>& v, long& off, const std::string& kernel, const std::string& bias,
                                   const std::string& ln, int groups, int K, int N, int act, double drop = 0.0, bool layer_norm = true,
                                   int Kt = 0, int Nt = 0) {
  DenseLn l{};
  if (!Kt) Kt = K;
  if (!Nt) Nt = N;
  l.Nt = Nt;
  const auto vec = [&](const std::string& name) { return add_leaf_box(v, off, name, groups, 1, Nt, 1, N); };
  l.W = add_leaf_box(v, off, kernel, groups, Kt, Nt, K, N);
  l.b = vec(bias);
  l.ln = layer_norm ? 1 : 0;
  l.g = layer_norm ? vec(ln + "/scale") : -1;
  l.be = layer_norm ? vec(ln + "/bias") : -1;
  l.w_gs = groups > 1 ? (long)K * N : 0; l.p_gs = groups > 1 ? N : 0; l.groups = groups; l.K = K; l.N = N; l.act = act;
  l.keep = drop > 0.0 ? (float)(1.0 - drop) : 0.f;
  return l;
}

struct DenseLnIo {   // one evaluation on `rows` rows per group
  const float* x; long ldx, x_gs;   // input [rows][K] (row stride ldx); group g's at x + g * x_gs (0: one input for all)
  float* y; long ld_y, y_goff;      // y[row * ld_y + g * y_goff + col]: column slices of a wider row, or one block per group
  float *xhat, *rstd;               // [groups * rows][N], [groups * rows]: what a backward pass reads, or nullptr (a plain layer keeps
                                    // its pre-activation in xhat and leaves rstd alone)
};
struct DenseLnGrad {   // one backward pass
  float* dy; long ld_dy, dy_goff;   // gradient wrt y, addressed like y (nullptr: the rank-1 form through the critic head)
  float *dpre, *dg;                 // [groups * rows][N] each: gradient wrt the Dense output, and dy * act' (a plain layer: the two
                                    // coincide, dpre alone is written and read)
};

// Y = X W as `splitk` K-split slabs behind `slabs` ([group][split][rows][N])
inline GemmDesc layer_fwd(const DenseLn& L, const float* P, const DenseLnIo& t, int rows, float* slabs, int splitk) {
  return gemm_fwd(t.x, t.ldx, t.x_gs, P + L.W, L.w_gs, slabs, L.groups, rows, L.N, L.K, splitk);
}
// the LayerNorm + activation launch that sums the slabs of `g` = layer_fwd(...)
inline LnFwdArgs layer_ln_fwd(const DenseLn& L, const float* P, const DenseLnIo& t, int rows, const GemmDesc& g,
                              const DenseLnDrop& site = DenseLnDrop{}) {
  LnFwdArgs l{};
  l.slabs = g.C; l.S = g.splitk; l.slab_stride = g.sCz;
  l.bias = P + L.b; l.pstride = L.p_gs;
  if (L.ln) { l.gamma = P + L.g; l.beta = P + L.be; }   // (else nullptr: the plain row)
  l.rows = L.groups * rows; l.rows_per_group = rows;
  l.y = t.y; l.ld_y = t.ld_y; l.y_goff = t.y_goff;
  l.xhat = t.xhat; l.rstd = t.rstd; l.act = L.act;
  l.d = L.Nt < L.N ? L.Nt : 0;
  l.drop = layer_drop(L, site);
  return l;
}
// The proprio branch runs its forward as one row kernel, without a GEMM (riders of the launch: the caller's)
inline ProprioArgs layer_row_fwd(const DenseLn& L, const float* P, const DenseLnIo& t) {
  return ProprioArgs{t.x, P + L.W, P + L.b, P + L.g, P + L.be, t.y, t.ld_y, t.xhat, t.rstd, nullptr, 0, nullptr, 0, 0};
}
// (site: the one the forward pass of these activations was given)
inline LnBwdArgs layer_ln_bwd(const DenseLn& L, const float* P, const DenseLnIo& t, const DenseLnGrad& d, int rows,
                              const DenseLnDrop& site = DenseLnDrop{}) {
  LnBwdArgs l{};
  l.dy = d.dy; l.ld_dy = d.ld_dy; l.dy_goff = d.dy_goff;
  l.y = t.y; l.ld_y = t.ld_y; l.y_goff = t.y_goff;
  l.xhat = t.xhat; l.rstd = t.rstd; l.pstride = L.p_gs;
  if (L.ln) { l.gamma = P + L.g; l.beta = P + L.be; }   // (else nullptr: the plain row, which writes dx alone)
  l.rows = L.groups * rows; l.rows_per_group = rows; l.D = L.N;
  l.dx = d.dpre; l.dg = d.dg; l.act = L.act;
  l.d = L.Nt < L.N ? L.Nt : 0;
  l.drop = layer_drop(L, site);
  return l;
}
// Gradients of the scale, shift and bias into G, a gradient vector indexed like the parameter vector.  A plain layer has the
// bias alone, the column sum of dpre (Colsum3Args mode 1): no dg or xhat is read, no scale or shift slot written.
inline Colsum3Args layer_colsum(const DenseLn& L, const DenseLnIo& t, const DenseLnGrad& d, int rows, float* G) {
  if (!L.ln) return Colsum3Args{d.dpre, nullptr, nullptr, L.groups, rows, L.N, nullptr, G + L.b, nullptr, L.p_gs, 1};
  return Colsum3Args{d.dg, t.xhat, d.dpre, L.groups, rows, L.N, G + L.g, G + L.be, G + L.b, L.p_gs, 0};
}
// Gradient of the kernel, written in place into G
inline GemmDesc layer_wgrad(const DenseLn& L, const DenseLnIo& t, const DenseLnGrad& d, int rows, float* G) {
  return gemm_wgrad(t.x, t.ldx, t.x_gs, d.dpre, L.N, (long)rows * L.N, G + L.W, L.N, L.w_gs, L.groups, L.K, L.N, rows);
}
// Gradient of the input: block z (= group * splitk + split) lands at out + z * out_zs with row stride ldo
inline GemmDesc layer_igrad(const DenseLn& L, const float* P, const DenseLnGrad& d, int rows, float* out, long ldo, long out_zs,
                            int splitk = 1) {
  return gemm_igrad(d.dpre, L.N, (long)rows * L.N, P + L.W, L.N, L.w_gs, out, ldo, out_zs, L.groups, rows, L.K, L.N, splitk);
}
// ... landing as the dy of the layer below
inline GemmDesc layer_igrad(const DenseLn& L, const float* P, const DenseLnGrad& d, int rows, const DenseLnGrad& below) {
  return layer_igrad(L, P, d, rows, below.dy, below.ld_dy, below.dy_goff);
}

// ---- the per-camera encoder head (resnet_v1.py:324-376, encoding.py:26-72): the encoder's own leaves (the SpatialLearnedEmbeddings
// kernel on the frozen trunk, or the SmallEncoder's convs), then Dense -> LayerNorm -> tanh.  first: camera 0's first leaf;
// camera k's leaves sit k * stride floats further.
struct CamHeadOffsets { long first, stride; DenseLn dense; };
// Appends enc/<k>/{what front("enc/<k>/") adds, dense/kernel, dense/bias, ln/scale, ln/bias} of n_cam cameras at `off`, which
// moves behind them: a [D][N] Dense and LayerNorm of width N.
template <typename F>
CamHeadOffsets add_cam_head_leaves(std::vector<Leaf>& v, long& off, int n_cam, int D, int N, F front) {
  CamHeadOffsets o{};
  for (int k = 0; k < n_cam; ++k) {
    const std::string p = "enc/" + std::to_string(k) + "/";
    const long first = off;
    front(p);
    const DenseLn l = add_dense_ln_leaves(v, off, p + "dense/kernel", p + "dense/bias", p + "ln", 1, D, N, kActTanh);
    if (k == 0) o = CamHeadOffsets{first, off - first, l};
  }
  o.dense.groups = n_cam; o.dense.w_gs = o.dense.p_gs = o.stride;
  return o;
}

}  // namespace serl
