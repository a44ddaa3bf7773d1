// csrc/last_error.hpp — the one way into crh_last_error()'s thread-local text from outside api.hip, which defines it. A header of its own,
// without <hip/hip_runtime.h>, because text.cpp is plain C++; the HIP translation units get it through api_internal.hpp.
#pragma once
#include <string>

namespace crh {
void set_last_error(const std::string& text);
}
