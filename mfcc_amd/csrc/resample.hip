// The sample-rate conversion kernels of libmfcc_hip.so (kernel_resample.hpp) as a translation
// unit, and so a device code object, of their own: mfcc_hip.hip only calls mfcc_rs::launch.
#define MFCC_RESAMPLE_DEFINE_KERNELS
#include "kernel_resample.hpp"
