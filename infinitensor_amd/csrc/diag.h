// Diagnostic hooks (clock stamps, timeline builds, ablations): switches that make a launch return wrong numbers on purpose. The shipped
// library never reads them; a diagnostic build (-DIROCM_DIAG: tools/diag_build.py) does.
#pragma once
#include <cstdlib>

namespace irocm {
inline const char *diag_getenv(const char *name) {
#ifdef IROCM_DIAG
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}
} // namespace irocm
