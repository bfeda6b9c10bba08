// Exponential moving average of a flat fp32 array, updated on the device (ema.hip): launch interface.
#pragma once
#include "common.h"

// pa_ema_state of include/poseadv.h.  updates: averaging steps applied so far; held: steps on which the optimizer's flag said "no step
// was taken" and the average stayed; apply, w, decay_used: what the LAST prologue decided, read by the lerp launches behind it.
struct PaEmaState { int updates, held, apply, reserved; float w, decay_used, reserved_f[2]; };

// one thread: skip_flag (NULL, or word 0 of an optimizer's device state) non-zero -> apply = 0, held += 1; else
// d = warmup ? min(decay, (1 + updates) / (10 + updates)) : decay in double, w = (float)(1.0 - d), decay_used = (float)d, apply = 1, updates += 1
int pa_launch_ema_advance(PaEmaState* s, float decay, int warmup, const int* skip_flag, hipStream_t st);
// apply == 0: nothing.  Else per element ema = copy ? src : fmaf(w, src - ema, ema).  ema and src 16-byte aligned, n > 0.
int pa_launch_ema_lerp(float* ema, const float* src, size_t n, const PaEmaState* s, bool copy, hipStream_t st);
int pa_ema_read_counts(const PaEmaState* s, long long* updates, long long* held, hipStream_t st);      // synchronises st
int pa_launch_ema_set_updates(PaEmaState* s, int updates, hipStream_t st);
