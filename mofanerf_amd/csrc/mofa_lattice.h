// The sample lattice of the geometry export, shared by the extraction (mofa_mesh.hip) and the vertex refinement (mofa_refine.hip): one
// coordinate formula, one inside test and one table of edge directions, so that a point named by an edge id is the same bits everywhere.
#pragma once
#include "mofa_common.h"

namespace mofa {
namespace {

__device__ __forceinline__ float grid_coord(float lo, float step, long long i) { return __fadd_rn(lo, __fmul_rn((float)i, step)); }

__device__ __forceinline__ bool inside(float s, float level) { return s >= level; }     // (false for NaN)

// the 7 lattice directions +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z of edge_id = 7 idx + dir
__device__ __constant__ int kDirDx[7] = {1, 0, 0, 1, 1, 0, 1};
__device__ __constant__ int kDirDy[7] = {0, 1, 0, 1, 0, 1, 1};
__device__ __constant__ int kDirDz[7] = {0, 0, 1, 0, 1, 1, 1};

}  // namespace
}  // namespace mofa
