// The delta kernel of the wide stream banks (kernel_stream_bank_online.hpp: online_deltas_wide_kernel, DESIGN.md section
// 6c-sexies) as a translation unit, and so a device code object, of its own: mfcc_hip.hip only calls
// mfcc_online::launch_deltas_wide, and the code object of the MFCC kernels is what it is without it.
#define MFCC_ONLINE_WIDE_UNIT
#include "kernel_stream_bank_online.hpp"
