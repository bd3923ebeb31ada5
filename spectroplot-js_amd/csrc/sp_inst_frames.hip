// One translation unit per FFT size of k_frames (compiled with -DSP_INST_FRAMES_LOG2N=6..13): the per-n launcher and its 12 variants
// (I/Q or L/R split x six loaders: 1-, 2-, 3-, 4-, 8-byte samples one frame ahead, or the checked generic loader), and the same 12
// variants of k_frames_batch with their launcher.
#include "sp_kernel_frames_batch.h"
