// Explicit instantiations of the pipelined convolution kernel: the low-register form (two blocks per CU), 32-channel waves.
#include "conv_pipe.h"
namespace dvfp {
DVF_PIPE_FAMILY_LR(1, 1, 1)
DVF_PIPE_FAMILY_LR(1, 2, 1)
}  // namespace dvfp
