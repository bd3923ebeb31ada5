// One translation unit per FFT size of k_frames_power (compiled with -DSP_INST_POWER_LOG2N=6..10): the per-n launcher and its 12
// variants (I/Q or L/R split x six loaders), beside the units of the other frame-loop kernels, whose code it leaves alone.
#include "sp_kernel_frames_power.h"
