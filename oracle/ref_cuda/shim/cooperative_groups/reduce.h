// Stand-in for <cooperative_groups/reduce.h>: the reference includes it and uses nothing from it.
#pragma once
#include "../cooperative_groups.h"
