// Stand-in for <cub/device/device_radix_sort.cuh> (see ../cub.cuh).
#pragma once
#include "../cub.cuh"
