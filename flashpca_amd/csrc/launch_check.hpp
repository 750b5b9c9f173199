// launch_check.hpp -- PRIVATE to libfpca.so: the check every launch wrapper makes after hipLaunchKernelGGL.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "common.hpp"

namespace fpca {

// a launch the runtime refused (bad grid, too much LDS, no code object for the device) -> Error(FPCA_EHIP)
inline void launch_check()
{
   const hipError_t e = hipGetLastError();
   if (e != hipSuccess) throw Error(-3, std::string("kernel launch failed: ") + hipGetErrorString(e));
}

} // namespace fpca
