// abi.hip -- ABI version of libmodex_hip.so (see include/modex_hip.h).  The library keeps no caller-observable mutable state:
// every entry point is a function of its arguments and the stream it is given, and none reads the environment
// (tests/test_abi.py).  The only statics are per-DEVICE latches of an idempotent driver call
// (hipFuncAttributeMaxDynamicSharedMemorySize, common.h:mx_set_dyn_lds).
#include "common.h"
MX_EXPORT int mx_abi_version(void) { return 21; }
