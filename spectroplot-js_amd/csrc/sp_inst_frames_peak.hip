// One translation unit per FFT size of k_frames_peak (compiled with -DSP_INST_PEAK_LOG2N=6..10): the per-n launcher and its 12 variants
// (I/Q or L/R split x six loaders), beside the units of k_frames / k_frames_batch (sp_inst_frames.hip), whose code it leaves alone.
#include "sp_kernel_frames_peak.h"
