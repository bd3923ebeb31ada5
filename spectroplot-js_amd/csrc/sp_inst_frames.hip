// The translation unit of the frame-loop kernels, compiled once per kernel family and FFT size: -DSP_INST_<FAMILY>_LOG2N=<L> selects the
// per-n launcher that is defined (each header defines its own under that macro), and the launcher instantiates its kernel's variants
// (I/Q or L/R split x six loaders: 1-, 2-, 3-, 4-, 8-byte samples one frame ahead, or the checked generic loader).  FRAMES: k_frames and
// k_frames_batch; PEAK, TRACES, POWER, INDEX: the kernel of that name.  The Makefile lists the families and their sizes.
#include "sp_kernel_frames_batch.h"
#include "sp_kernel_frames_index.h"
#include "sp_kernel_frames_peak.h"
#include "sp_kernel_frames_power.h"
#include "sp_kernel_frames_traces.h"
