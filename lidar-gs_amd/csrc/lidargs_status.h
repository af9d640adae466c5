// lidargs_status.h -- the last-error message and the launch check of the libraries that are one source each (adam.hip,
// decode_options.hip, raydrop_mlp.hip, range_view.hip).  Host code only.  Everything has internal linkage: each of those libraries is a
// single translation unit, so each gets a message buffer of its own, which its *_last_error() entry point returns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

namespace {

thread_local char g_err[256] = "";

// Records "<what>: <msg><detail>" and returns `code`.
int fail(int code, const char* what, const char* msg, const char* detail = "") {
    snprintf(g_err, sizeof g_err, "%s: %s%s", what, msg, detail);
    return code;
}

// Directly behind the launches of an entry point: 0, or records "<what>: <stage><HIP's error string>" and returns `code`.
int launched(int code, const char* what, const char* stage = "launch: ") {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(code, what, stage, hipGetErrorString(e));
}

}  // namespace
