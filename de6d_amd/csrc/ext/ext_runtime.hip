// ext_runtime.hip — library identification and error bookkeeping for libdet6d_hip_ext.so (what runtime.hip is to
// libdet6d_hip.so; declared in ext_common.h and include/det6d_ext.h).
#include "../common.h"
#include "../../../include/det6d_ext.h"
#include "ext_common.h"
#include <stdarg.h>
#include <stdio.h>

namespace {
thread_local char g_ext_err[256] = "";
}

void det6d_set_error(const char *what, hipError_t err) {
  snprintf(g_ext_err, sizeof(g_ext_err), "%s: %s", what, hipGetErrorString(err));
}

int det6d_ext_fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_ext_err, sizeof(g_ext_err), fmt, ap);
  va_end(ap);
  return DET6D_EINVAL;
}

DET6D_API const char *det6d_ext_version(void) { return "det6d-hip-ext gfx950 ext3"; }
DET6D_API const char *det6d_ext_last_error(void) { return g_ext_err; }
