// Stand-in for <cub/cub.cuh>: hipCUB under the name cub.
#pragma once
#include <hipcub/hipcub.hpp>
namespace cub = hipcub;
