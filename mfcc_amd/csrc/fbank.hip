// The filterbank kernels of libmfcc_hip.so (kernel_fbank.hpp) as a translation unit, and so a
// device code object, of their own: mfcc_hip.hip only calls mfcc_fbank::launch_generic and mfcc_fbank::launch_fused.
// MFCC_NO_LAUNCHERS: the headers kernel_fbank.hpp builds on give their device helpers and tables here, not their kernels.
#define MFCC_FBANK_DEFINE_KERNELS
#define MFCC_NO_LAUNCHERS
#include "kernel_fbank.hpp"
