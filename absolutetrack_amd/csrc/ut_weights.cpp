// Checkpoint blob -> folded, canonicalised, packed host tensors (ut_weights.h).  No device code and no runtime call.
#include "ut_weights.h"

#include <math.h>

#include "ut_split_pack.h"

namespace ut {
namespace {

// A short blob ends the walk: take() returns null from then on and whoever is about to read the pointers checks `ok` once.
struct Cursor {
  const float* p;
  size_t left;
  const float* take(size_t n) {
    if (n > left) { left = 0; ok = false; return nullptr; }
    const float* r = p; p += n; left -= n; return r;
  }
  bool ok = true;
};

struct BN { const float *g = nullptr, *b = nullptr, *m = nullptr, *v = nullptr; };

BN take_bn(Cursor& c, int ch) {
  BN bn;
  bn.g = c.take(ch); bn.b = c.take(ch); bn.m = c.take(ch); bn.v = c.take(ch);
  c.take(1);   // num_batches_tracked
  return bn;
}

Folded fold_conv(const float* w, const float* conv_bias, const BN* bn, int cin, int cout, int taps) {
  Folded f;
  f.cin = cin; f.cout = cout; f.taps = taps;
  f.w.resize((size_t)cout * cin * taps);
  f.b.resize(cout);
  for (int o = 0; o < cout; ++o) {
    double s = 1.0, shift = conv_bias ? (double)conv_bias[o] : 0.0;
    if (bn) {
      s = (double)bn->g[o] / sqrt((double)bn->v[o] + 1e-5);
      shift = (shift - (double)bn->m[o]) * s + (double)bn->b[o];
    }
    f.b[o] = (float)shift;
    for (size_t i = (size_t)o * cin * taps; i < (size_t)(o + 1) * cin * taps; ++i) f.w[i] = (float)((double)w[i] * s);
  }
  return f;
}

// ---- channel canonicalisation (exact: powers of two only) --------------------------------------------------------------
// relu(bn(conv)) commutes with a positive per-channel factor, and a power of two commutes with every fp32 rounding
// (lib/models/backbone_resnet.py:56-72): scaling output channel c of a producer (its folded weight row and bias) by 2^k
// and input channel c of every consumer (its weight column) by 2^-k leaves every later fp32 value bit for bit as it was.
// A checkpoint fixes the scale of an inner channel only up to that freedom (a near-dead BatchNorm channel and the large
// consumer weights that compensate it are the same function as a well-scaled pair), while the split-fp16 arithmetic keeps
// ONE power-of-two scale per activation tensor and ONE per weight tensor: a channel 2^-18 below its tensor's largest has a
// subnormal second piece.  So every channel is brought to a canonical scale at pack time: 2^k_c puts the largest magnitude
// among the channel's producer rows (weights and bias) into [1, 2).  Two networks that differ by per-channel powers of two
// pack to the same tensors, in both arithmetics.
float row_max(const Folded& f, int o) {
  float m = fabsf(f.b[o]);
  const size_t n = (size_t)f.cin * f.taps;
  for (size_t i = 0; i < n; ++i) {
    const float a = fabsf(f.w[(size_t)o * n + i]);
    m = a > m ? a : m;          // (a NaN never raises m: such a row keeps its scale)
  }
  return m;
}
int octave_shift(float m) {       // k with m * 2^k in [1, 2); 0 when the row is all zeros or not finite
  if (!(m > 0.f) || !(m < INFINITY)) return 0;
  return -ilogbf(m);
}
void scale_row(Folded& f, int o, int k) {
  if (!k) return;
  const size_t n = (size_t)f.cin * f.taps;
  for (size_t i = 0; i < n; ++i) f.w[(size_t)o * n + i] = ldexpf(f.w[(size_t)o * n + i], k);
  f.b[o] = ldexpf(f.b[o], k);
}
void scale_col(Folded& f, int c, int k) {
  if (!k) return;
  for (int o = 0; o < f.cout; ++o)
    for (int t = 0; t < f.taps; ++t) {
      float& v = f.w[((size_t)o * f.cin + c) * f.taps + t];
      v = ldexpf(v, k);
    }
}
// Channel c of one activation tensor: `keys` (a subset of its producers) define 2^k_c, every producer's row c is scaled by it
// and every consumer's column c by its inverse.
void canonicalise_channels(const std::vector<Folded*>& keys, const std::vector<Folded*>& producers,
                           const std::vector<Folded*>& consumers) {
  const int ch = keys[0]->cout;
  for (int c = 0; c < ch; ++c) {
    float m = 0.f;
    for (Folded* p : keys) { const float r = row_max(*p, c); m = r > m ? r : m; }
    const int k = octave_shift(m);
    for (Folded* p : producers) scale_row(*p, c, k);
    for (Folded* q : consumers) scale_col(*q, c, -k);
  }
}

// the same convolution with zero rows / columns up to cout x cin channels
Folded pad_channels(const Folded& f, int cin, int cout) {
  Folded g;
  g.cin = cin; g.cout = cout; g.taps = f.taps;
  g.w.assign((size_t)cout * cin * f.taps, 0.f);
  g.b.assign(cout, 0.f);
  for (int o = 0; o < f.cout; ++o) {
    g.b[o] = f.b[o];
    for (int c = 0; c < f.cin; ++c)
      for (int t = 0; t < f.taps; ++t) g.w[((size_t)o * cin + c) * f.taps + t] = f.w[((size_t)o * f.cin + c) * f.taps + t];
  }
  return g;
}

bool fold_block(Cursor& c, FoldedBlock& fb, int cin, int cout, int stride, bool ds) {
  const float* w1 = c.take((size_t)cout * cin * 9);
  BN bn1 = take_bn(c, cout);
  const float* w2 = c.take((size_t)cout * cout * 9);
  BN bn2 = take_bn(c, cout);
  const float* wd = nullptr;
  BN bnd;
  if (ds) { wd = c.take((size_t)cout * cin); bnd = take_bn(c, cout); }
  if (!c.ok) return false;
  fb.stride = stride; fb.has_ds = ds;
  fb.conv1 = fold_conv(w1, nullptr, &bn1, cin, cout, 9);
  fb.conv2 = fold_conv(w2, nullptr, &bn2, cout, cout, 9);
  if (ds) fb.ds = fold_conv(wd, nullptr, &bnd, cin, cout, 1);
  return true;
}

// the block's inner channels: conv1 writes them, conv2 reads them (conv1's input channels must have their final scale)
void canonicalise_inner(FoldedBlock& fb) { canonicalise_channels({&fb.conv1}, {&fb.conv1}, {&fb.conv2}); }

bool fold_backbone(Cursor& c, FoldedBackbone& out) {
  // stem (lib/models/model_utils.py:119-124)
  const float* sw = c.take(32 * 9);
  const float* sb = c.take(32);
  BN sbn = take_bn(c, 32);
  if (!c.ok) return false;
  Folded& stem = out.stem;
  Folded& proj = out.proj;
  FoldedBlock* fb = out.fb;
  stem = fold_conv(sw, sb, &sbn, 1, 32, 9);
  // ResNet layers "2352", planes 32/64/128/256, strides 1/2/2/2 (lib/models/backbone_resnet.py:168-192)
  const int nb[4] = {2, 3, 5, 2}, planes[4] = {32, 64, 128, 256}, strides[4] = {1, 2, 2, 2};
  int first_of_layer[5] = {0, 0, 0, 0, 12};
  int cin = 32, bi = 0;
  for (int l = 0; l < 4; ++l) {
    first_of_layer[l] = bi;
    for (int k = 0; k < nb[l]; ++k) {
      int st = k == 0 ? strides[l] : 1;
      bool ds = k == 0 && (st != 1 || cin != planes[l]);
      if (!fold_block(c, fb[bi++], cin, planes[l], st, ds)) return false;
      cin = planes[l];
    }
  }
  const float* pw = c.take(72 * 256); const float* pb = c.take(72);
  if (!c.ok) return false;
  proj = fold_conv(pw, pb, nullptr, 256, 72, 1);
  // Canonical channel scales, fixed in network order so that each one is defined by tensors whose input side is final
  // already (two checkpoints that differ by per-channel powers of two then arrive at the same tensors):
  //  - the TRUNK of a layer (the tensor its identity shortcuts carry through the blocks): channel c is written by conv2 of
  //    every block of the layer and by the first block's shortcut convolution (layer1: by the stem) and read by conv1 of the
  //    layer's later blocks and by whatever enters the next layer (its first block's conv1 and shortcut convolution; after
  //    layer4: the projection, whose 72 outputs are the features of the ABI and keep their scale).  Its scale comes from the
  //    rows that write the trunk's FIRST tensor: the stem's, or the first block's shortcut and conv2 rows;
  //  - the inner channels of every block, once the block's input has its scale.
  for (int l = 0; l < 4; ++l) {
    const int b0 = first_of_layer[l], b1 = l < 3 ? first_of_layer[l + 1] : 12;
    std::vector<Folded*> keys, prod, cons;
    if (fb[b0].has_ds) {
      canonicalise_inner(fb[b0]);             // its input is the previous layer's trunk: final
      keys = {&fb[b0].ds, &fb[b0].conv2};
      prod = {&fb[b0].ds};
    } else {
      keys = {&stem};
      prod = {&stem};
      cons.push_back(&fb[b0].conv1);
    }
    for (int b = b0; b < b1; ++b) {
      prod.push_back(&fb[b].conv2);
      if (b > b0) cons.push_back(&fb[b].conv1);
    }
    if (l < 3) { cons.push_back(&fb[b1].conv1); cons.push_back(&fb[b1].ds); }
    else cons.push_back(&proj);
    canonicalise_channels(keys, prod, cons);
    for (int b = fb[b0].has_ds ? b0 + 1 : b0; b < b1; ++b) canonicalise_inner(fb[b]);
  }
  return true;
}

// two BasicBlocks of ch channels, then the ch -> d output convolution that follows the average pool
bool fold_regressor(Cursor& c, FoldedRegressor& r, int ch, int d) {
  r.c = ch; r.d = d;
  for (int i = 0; i < 2; ++i) {
    FoldedBlock& fb = r.blocks[i];
    if (!fold_block(c, fb, ch, ch, 1, false)) return false;
    canonicalise_inner(fb);
    r.wide[i].conv1 = pad_channels(fb.conv1, kRegSplitCh, kRegSplitCh);
    r.wide[i].conv2 = pad_channels(fb.conv2, kRegSplitCh, kRegSplitCh);
  }
  const float* w = c.take((size_t)d * ch);
  const float* b = c.take(d);
  if (!c.ok) return false;
  r.w_out.assign(w, w + (size_t)d * ch);
  r.b_out.assign(b, b + d);
  return true;
}

}  // namespace

bool fold_network(const float* blob, size_t n, FoldedNetwork& out) {
  Cursor c{blob, n};
  if (!fold_backbone(c, out.backbone)) return false;
  // fusion 144 -> 108 -> 72 -> 72 (lib/models/model_utils.py:141-163)
  const float* w0 = c.take(108 * 144); const float* b0 = c.take(108); BN bn0 = take_bn(c, 108);
  const float* w1 = c.take(72 * 108); const float* b1 = c.take(72); BN bn1 = take_bn(c, 72);
  const float* w2 = c.take(72 * 72); const float* b2 = c.take(72);
  // temporal 90 -> 90 x3 (lib/models/temporal.py:31-38)
  const float *tw[3], *tb[3];
  for (int i = 0; i < 3; ++i) { tw[i] = c.take(90 * 90); tb[i] = c.take(90); }
  // skeleton encoder (lib/models/skeleton_encoder.py:36-41)
  const float* lw = c.take(144 * 132); const float* lb = c.take(144); BN bn = take_bn(c, 4);
  if (!c.ok) return false;
  out.fusion[0] = fold_conv(w0, b0, &bn0, 144, 108, 1);
  out.fusion[1] = fold_conv(w1, b1, &bn1, 108, 72, 1);
  out.fusion[2] = fold_conv(w2, b2, nullptr, 72, 72, 1);
  for (int i = 0; i < 3; ++i) out.temporal[i] = fold_conv(tw[i], tb[i], nullptr, 90, 90, 1);
  out.skel_w.assign(lw, lw + 144 * 132);
  out.skel_b.assign(lb, lb + 144);
  out.skel_scale.resize(4); out.skel_shift.resize(4);
  for (int k = 0; k < 4; ++k) {
    double s = (double)bn.g[k] / sqrt((double)bn.v[k] + 1e-5);
    out.skel_scale[k] = (float)s; out.skel_shift[k] = (float)((double)bn.b[k] - (double)bn.m[k] * s);
  }
  return fold_regressor(c, out.reg_k, 76, 62) && fold_regressor(c, out.reg_u, 72, 63) && c.left == 0;
}

// Pack folded weights to [cout_pad][k_pad] with k = slice*(taps*cslice) + tap*cslice + c (see ut_kernels.h).
PackedConv pack_conv_host(const Folded& f, int ksize, int stride, int cout_store, bool pw_fragments) {
  PackedConv cw;
  const int cin = f.cin, cout = f.cout;
  cw.cin = cin; cw.cout = cout; cw.ksize = ksize; cw.stride = stride;
  cw.pad = ksize == 3 ? 1 : 0;
  cw.taps = ksize * ksize;
  cw.cin_pad = round_up(cin, 4);
  cw.cout_store = cout_store;
  cw.cout_pad = round_up(cout_store, 128);
  cw.k_total = cw.taps * cw.cin_pad;
  cw.cslice = cw.cin_pad % 32 == 0 ? 32 : cw.cin_pad;
  cw.k_pad = round_up(cw.k_total, 32);
  cw.flops_per_pixel = 2.0 * cw.taps * cin * cout;
  std::vector<float>& wp = cw.wp;
  std::vector<float>& bp = cw.bp;
  wp.assign((size_t)cw.cout_pad * cw.k_pad, 0.f);
  bp.assign(cw.cout_pad, 0.f);
  for (int o = 0; o < cout; ++o) {
    bp[o] = f.b[o];
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < cw.taps; ++t)
        wp[(size_t)o * cw.k_pad + (c / cw.cslice) * (cw.taps * cw.cslice) + t * cw.cslice + c % cw.cslice] =
            f.w[((size_t)o * cin + c) * cw.taps + t];
  }
  {
    double ws = 0.0, bm = 0.0;
    for (int o = 0; o < cout; ++o) {
      double rs = 0.0;
      for (int k = 0; k < cw.k_pad; ++k) rs += fabs((double)wp[(size_t)o * cw.k_pad + k]);
      ws = rs > ws ? rs : ws;
      bm = fabs((double)bp[o]) > bm ? fabs((double)bp[o]) : bm;
    }
    cw.wsum_rows = (float)(ws * 1.0001);
    cw.bias_max = (float)(bm * 1.0001);
  }
  // fp16 planes for the split-fp16 kernels: the layers they take (channel slice == chunk width, >= 6 chunks: the 3x3
  // convolutions of the backbone; conv_split.hip from 64 channels out, conv_patch.hip's split instantiation for layer1)
  // (and the 1x1 stride-2 shortcut of a 32-channel input: conv_c32s2.hip computes it beside the block's first convolution)
  if (cw.cslice == 32 && (cw.k_pad / 32 >= 6 || (ksize == 1 && stride == 2 && cw.cin_pad == 32)) && cw.cout_store >= 32 && cw.cout_store % 4 == 0) {
    cw.planes.resize((size_t)2 * cw.cout_pad * cw.k_pad);
    const float scale = split_weight_scale(wp.data(), wp.size());
    cw.split_unscale = 1.0f / scale;
    pack_split_weights(wp.data(), cw.cout_pad, cw.k_pad, scale, cw.planes.data());
  }
  // 1x1 convolutions that run on conv_pw.hip: the same matrix in the order conv_pw.hip's lanes consume it - [32-row block][8-wide k step][lane][4]
  // with lane (fr = lane & 31, fh = lane >> 5) holding row 32 n + fr, k = 8 s + 4 fh .. + 3 -, so that a wave's fragment of a step
  // is one contiguous kilobyte
  if (pw_fragments && ksize == 1) {
    cw.wfrag.resize(wp.size());
    const int steps = cw.k_pad / 8;
    for (int n = 0; n < cw.cout_pad / 32; ++n)
      for (int st = 0; st < steps; ++st)
        for (int lane = 0; lane < 64; ++lane)
          for (int c = 0; c < 4; ++c)
            cw.wfrag[(((size_t)n * steps + st) * 64 + lane) * 4 + c] =
                wp[(size_t)(32 * n + (lane & 31)) * cw.k_pad + 8 * st + 4 * (lane >> 5) + c];
  }
  return cw;
}

}  // namespace ut
