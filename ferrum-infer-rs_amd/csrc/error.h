// Thread-local error text returned by ferrum_hip_last_error(); set_error / last_error are defined in abi.cc.  Host-only: no HIP header needed.
#pragma once

namespace fh {
void set_error(const char* fmt, ...);
const char* last_error();
}  // namespace fh

#define FH_REQUIRE(cond, ...)                 \
    do {                                      \
        if (!(cond)) {                        \
            fh::set_error(__VA_ARGS__);       \
            return 2;                         \
        }                                     \
    } while (0)
