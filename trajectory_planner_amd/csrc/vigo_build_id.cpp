// vigo_build_id.cpp — vigo_build_id() (include/vigo.h).  Compiled and linked last: VIGO_BUILD_ID comes from the Makefile,
// digests of the compiled code of every other object of the library (build_id.py).
#include "vigo.h"

const char* vigo_build_id(void) { return VIGO_BUILD_ID; }
