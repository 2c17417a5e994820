// What conv_strided.hip (the stride-2 kernels) borrows from conv_wgrad.hip: the packed partial-sum layout of the split-bf16 weight
// gradient and its unpack.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace cd {

// packed [split][co 16][ci 16][tap][16][16] of wgrad_split.hip for (Cout, Cin, ks): 16-channel tiles, the largest number of slices
// the workspace of cd_conv2d_wgrad_workspace_floats has room for in the split arithmetic modes, floats per slice
void wgrad_split_layout_info(int Cout, int Cin, int ks, int* cogs, int* cigs, int* max_splits, size_t* slice);

// dw[groups][Cout][Cin][ks][ks] (+)= the `splits` slices of every group's workspace, added in the fixed order of unpack_wgrad_kernel
int launch_unpack_wgrad_split(const float* workspace, int Cout, int Cin, int ks, int cigs, int splits, size_t slice, float* dw, int accumulate,
                              int groups, size_t ws_group_stride, hipStream_t s);

}  // namespace cd
