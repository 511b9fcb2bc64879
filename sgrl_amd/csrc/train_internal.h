// train_internal.h -- what the sources behind include/sgrl_train.h share: the one error string sgrl_train_last_error() returns
// (thread local, defined in train_gemm.hip) and the check behind a launch.
#ifndef SGRL_TRAIN_INTERNAL_H
#define SGRL_TRAIN_INTERNAL_H

#include <string>

namespace sgrl_train_detail {
int fail(int code, const std::string& msg);       // sets the message, returns code
bool launched(const char* what, int* rc);         // hipGetLastError behind a launch; false: *rc = SGRL_ERR_HIP, message set
}  // namespace sgrl_train_detail

#endif
