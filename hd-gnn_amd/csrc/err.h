// err.h -- the library's per-thread error message (hdg_last_error) and the helper every
// entry point reports failures through.  No HIP header in reach: host-only sources (ckpt.cpp)
// include this alone.
#ifndef HDGNN_ERR_H
#define HDGNN_ERR_H

#include <stdarg.h>
#include <stdio.h>

namespace hdg {

inline thread_local char g_err[512] = "";

// formats the message into g_err and returns code
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

}  // namespace hdg

#endif  // HDGNN_ERR_H
