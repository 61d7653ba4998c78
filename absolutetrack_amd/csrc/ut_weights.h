// The checkpoint blob as the tensors the kernels read: BatchNorm folding, channel canonicalisation, the packed convolution
// layout.  Host arithmetic on host vectors only: no device, no handle (ut_api.hip uploads the results).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace ut {

constexpr int kRegSplitCh = 128;   // channels of the regressor's tensors when its convolutions run in split-fp16 (zero padded)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// One convolution with eval-mode BatchNorm (eps 1e-5) folded in, as the reference's tensors lay it out:
//   y = s*(conv(x)+b-mean)+beta,  s = gamma/sqrt(var+eps)   ->   w[o][c][t] * s[o],  bias[o] = (b-mean)*s+beta
// (fold in double, one rounding to fp32).
struct Folded {
  std::vector<float> w;      // [cout][cin][taps]
  std::vector<float> b;      // [cout]
  int cin = 0, cout = 0, taps = 0;
};

// A BasicBlock's folded convolutions.
struct FoldedBlock {
  Folded conv1, conv2, ds;
  bool has_ds = false;
  int stride = 1;
};

// stem + ResNet "2352" + projection, folded, with canonical channel scales
struct FoldedBackbone {
  Folded stem, proj;
  FoldedBlock fb[12];
};

struct FoldedRegressor {
  FoldedBlock blocks[2];     // inner channels canonical
  FoldedBlock wide[2];       // the same convolutions with input and output channels zero-padded to kRegSplitCh
  std::vector<float> w_out;  // [d][c] raw (applied after the average pool)
  std::vector<float> b_out;  // [d]
  int c = 0, d = 0;
};

struct FoldedNetwork {
  FoldedBackbone backbone;
  Folded fusion[3];          // 144 -> 108 -> 72 -> 72
  Folded temporal[3];        // 90 -> 90
  std::vector<float> skel_w, skel_b;          // [144][132], [144] raw
  std::vector<float> skel_scale, skel_shift;  // [4]: the skeleton encoder's BatchNorm as y = x * scale + shift
  FoldedRegressor reg_k, reg_u;               // known / unknown skeleton
};

// One walk over the blob in checkpoint order.  False exactly when the walk does not consume n floats.
bool fold_network(const float* blob, size_t n, FoldedNetwork& out);

struct ConvGeom {
  int cin = 0, cin_pad = 0, cout = 0, cout_pad = 0, cout_store = 0;
  int taps = 1, ksize = 1, stride = 1, pad = 0, k_total = 0, k_pad = 0, cslice = 0;
  double flops_per_pixel = 0;   // 2 * taps * cin * cout, un-padded
};

struct PackedConv : ConvGeom {
  std::vector<float> wp;          // [cout_pad][k_pad], k = slice*(taps*cslice) + tap*cslice + c (see ut_kernels.h)
  std::vector<float> bp;          // [cout_pad]
  std::vector<float> wfrag;       // on request, 1x1 only: wp as [cout_pad / 32][k_pad / 8][64 lanes][4], conv_pw.hip's fragment order; else empty
  std::vector<uint16_t> planes;   // the two fp16 planes of wp * 2^k in fragment order (conv_split.hip); empty: not a split-fp16 layer
  float split_unscale = 0.f;      // 2^-k
  float wsum_rows = 0.f;          // max over output channels of sum_k |w| (folded), rounded up: bounds |conv(x)| by wsum_rows * max|x|
  float bias_max = 0.f;           // max |bias| (folded)
};

// pw_fragments (1x1 only): also fill wfrag, for the convolutions that conv_pw.hip takes
PackedConv pack_conv_host(const Folded& f, int ksize, int stride, int cout_store, bool pw_fragments = false);

}  // namespace ut
