// Error reporting of the C ABI (thread-local message, never throws, never allocates on the device) and the run-time options.
#include "common.hpp"
#include "options.hpp"
#include <stdarg.h>
#include <string.h>

static thread_local char g_err[512] = "";

void pero_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* pero_last_error(void) { return g_err; }
extern "C" int pero_abi_version(void) { return 2; }  // 2: pero_gemm takes a caller-owned workspace (round 3)

PeroOptions g_opt;
static const struct { const char* name; int PeroOptions::*field; const char* meaning; } g_option_table[] = {
#define X(name_, default_, meaning_) {#name_, &PeroOptions::name_, meaning_},
  PERO_OPTIONS(X)
#undef X
};
extern "C" int pero_set_option(const char* name, int value) {
  for (const auto& o : g_option_table)
    if (name && !strcmp(name, o.name)) {
      g_opt.*o.field = value;
      if (g_opt.splitk_items <= 0) g_opt.splitk_items = 512;   // the one special case: no work-item target = the default
      return PERO_OK;
    }
  pero_set_error("pero_set_option: unknown option %s", name ? name : "(null)");
  return PERO_E_INVALID;
}
