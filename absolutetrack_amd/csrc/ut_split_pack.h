// Host side of the split-fp16 weight format (conv_split.hip defines both: the fragment order belongs with the kernel that reads
// it).  Plain C++: shared by the kernel interface (ut_kernels.h) and the host-only weight packing (ut_weights.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ut {

size_t pack_split_weights(const float* w, int cout_pad, int k_pad, float scale, uint16_t* out);
float split_weight_scale(const float* w, size_t n);

}  // namespace ut
