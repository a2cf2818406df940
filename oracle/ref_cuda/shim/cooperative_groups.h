// Stand-in for <cooperative_groups.h>: HIP ships the same namespace.
#pragma once
#include <hip/hip_cooperative_groups.h>
