/* A four-entry-point C ABI in the style of include/ia_amd.h, for tests/test_binding_cpu.py: the loader of intrinsicavatar_amd/_lib.py
 * reads THIS header and binds tests/binding_stub.c, so the marshalling is checked without libia_amd.so and without a GPU. */
#ifndef BINDING_STUB_H
#define BINDING_STUB_H

#include <stddef.h>
#include <stdint.h>

typedef void* ia_stream_t;

const char* ia_last_error(void);

/* writes what it received into out[9]: n, dev (address), f, d, u, z, host (address), host[1] (0 when host is NULL), stream (address) */
int ia_stub_echo(int64_t n, const void* dev, float f, double d, uint32_t u, size_t z, const float* host, double* out, ia_stream_t stream);

/* sets the error text "stub: refused <n>" and returns -3 */
int ia_stub_fail(int64_t n, ia_stream_t stream);

/* host-only query: 16 * n - 3 (negative for n = 0: a value, not a status) */
int64_t ia_stub_tmp_bytes(int64_t n);

#endif
