// The library behind tests/binding_stub.h: entry points that record their arguments, fail on request, or answer a size query.
// Built by tests/test_binding_cpu.py with gcc and loaded through intrinsicavatar_amd/_lib.py's loader.
#include <stdio.h>

#include "binding_stub.h"

#define EXPORT __attribute__((visibility("default")))

static char g_err[128] = "";

EXPORT const char* ia_last_error(void) { return g_err; }

EXPORT int ia_stub_echo(int64_t n, const void* dev, float f, double d, uint32_t u, size_t z, const float* host, double* out, ia_stream_t stream) {
    out[0] = (double)n;
    out[1] = (double)(uintptr_t)dev;
    out[2] = (double)f;
    out[3] = d;
    out[4] = (double)u;
    out[5] = (double)z;
    out[6] = (double)(uintptr_t)host;
    out[7] = host ? (double)host[1] : 0.0;
    out[8] = (double)(uintptr_t)stream;
    return 0;
}

EXPORT int ia_stub_fail(int64_t n, ia_stream_t stream) {
    (void)stream;
    snprintf(g_err, sizeof g_err, "stub: refused %lld", (long long)n);
    return -3;
}

EXPORT int64_t ia_stub_tmp_bytes(int64_t n) { return 16 * n - 3; }
