// ext_common.h — what the sources of libdet6d_hip_ext.so share besides csrc/common.h: the library's runtime, defined once
// in ext_runtime.hip.  Its error slot (det6d_ext_last_error) is written by det6d_ext_fail for a refused call and by
// det6d_set_error (declared in csrc/common.h) for a failed launch.
#pragma once

// formats the message of a refused call into the calling thread's error slot; returns DET6D_EINVAL
int det6d_ext_fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
