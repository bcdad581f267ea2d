// Dev-only: what `#include <hip/hip_runtime.h>` finds in the CPU builds of the equity kernels (tools/host_sim/equity_sim.cpp, compiled with
// -I tools/host_sim/stub -include tools/host_sim/wg_shim.h): nothing -- the shim has already supplied what the kernels use.
#pragma once
