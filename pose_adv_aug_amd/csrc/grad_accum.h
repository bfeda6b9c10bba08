// Gradient accumulation over micro-batches (grad_accum.hip; utils.optim._FlatOptimizer.accumulate): launch interface.
#pragma once
#include "common.h"

// dst[i] = b ? a[i] + b[i] : a[i] for i < n, one fp32 addition per element.  dst may be exactly a or exactly b (every thread reads the
// elements it writes before it writes them); any other overlap is the caller's to refuse (pa_grad_accumulate does).  All three pointers
// 16-byte aligned: 16-byte chunks; otherwise one element per thread and trip.  n > 0.
int pa_launch_grad_accumulate(float* dst, const float* a, const float* b, size_t n, hipStream_t st);
