// capi_error.h -- the host error path every C-ABI translation unit shares: a per-thread message buffer, fail() to fill
// it, and the check that follows a kernel launch.  Everything lives in an anonymous namespace, so each translation unit
// that includes this keeps a buffer of its own (spec_* and fno_* share a library and still report independently);
// its `<prefix>_last_error(void)` returns g_err.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

namespace {

thread_local char g_err[512] = "";

// records the message and returns `code`, so that a refusal reads `return fail(-1, "...", ...);`
[[maybe_unused]] int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// after a kernel launch: 0, or `code` with "<who> launch failed: <hipGetErrorString>"
[[maybe_unused]] int launch_status(int code, const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(code, "%s launch failed: %s", who, hipGetErrorString(e));
}

}  // namespace
