// The centring kernels of libmfcc_hip.so (kernel_center.hpp) as a translation unit, and so a
// device code object, of their own: mfcc_hip.hip only calls mfcc_center::launch_dense and launch_ragged.
#define MFCC_CENTER_DEFINE_KERNELS
#include "kernel_center.hpp"
