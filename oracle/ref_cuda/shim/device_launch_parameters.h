// Stand-in for <device_launch_parameters.h>: threadIdx / blockIdx come with the HIP runtime.
#pragma once
#include "cuda_runtime.h"
