// Explicit instantiations of the pipelined convolution kernel: the low-register form, 64-channel waves.
#include "conv_pipe.h"
namespace dvfp {
DVF_PIPE_FAMILY_LR(2, 1, 1)
}  // namespace dvfp
