// The sample-decode kernels of libmfcc_hip.so (kernel_decode.hpp) as a translation unit, and so
// a device code object, of their own: mfcc_hip.hip only calls mfcc_decode::launch.
#define MFCC_DECODE_DEFINE_KERNELS
#include "kernel_decode.hpp"
