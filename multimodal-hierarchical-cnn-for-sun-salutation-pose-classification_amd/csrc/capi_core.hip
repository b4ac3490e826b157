// Library-wide C-ABI helpers: version, thread-local error text, the per-thread ordering event.
#include <stdarg.h>
#include <stdio.h>

#include "qt_common.h"

namespace {
thread_local char g_err[512] = "";
}

void qt_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

hipEvent_t qt_thread_event() {
  thread_local hipEvent_t ev = nullptr;
  thread_local int ev_dev = -1;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  if (ev && ev_dev != dev) {   // (an event belongs to the device it was created on)
    (void)hipEventDestroy(ev);
    ev = nullptr;
  }
  if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
  ev_dev = dev;
  return ev;
}

extern "C" int qt_version(void) { return 100; }
extern "C" const char* qt_last_error(void) { return g_err; }
