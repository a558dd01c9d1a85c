/* mex_int64.h — the int64 part of MATLAB's MX API for the TEST build of the
 * gateway against tests/mex_shim/mex.h, which declares double arrays only.
 * matlab/swrt_mex.cpp includes this file when it is on the include path (the
 * test build); under MATLAB it is not, and MATLAB's own mex.h provides
 * mxINT64_CLASS and mxGetInt64s.
 *
 * The shim's mxArray is untyped: mxCreateNumericArray ignores the class and
 * keeps 8-byte words, zeroed.  An int64 array therefore lives in the words of
 * what the shim calls a double array, and a test views the words it gets back
 * as int64 (tests/test_mex_kmap_series.py). */
#pragma once
#include <stdint.h>

#include "mex.h"

typedef int64_t mxInt64;
/* (the shim ignores the class; MATLAB's value, 14, is outside this enum's range) */
static const mxClassID mxINT64_CLASS = mxUNKNOWN_CLASS;

static inline mxInt64* mxGetInt64s(const mxArray* a) {
  /* (the same 8-byte words; never read as doubles by the gateway) */
  return (mxInt64*)(void*)mxGetDoubles(a);
}
