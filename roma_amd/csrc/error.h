// The library's error reporting, host only and without a HIP header: what common.h shares with the files a plain C++ compiler builds.
#pragma once
#include "../../include/roma_hip.h"

namespace roma {

void set_error(const char* fmt, ...);

#define ROMA_REQUIRE(cond, code, ...)            \
  do {                                           \
    if (!(cond)) {                               \
      ::roma::set_error(__VA_ARGS__);            \
      return (code);                             \
    }                                            \
  } while (0)

}  // namespace roma
