// om_bvh.h — host BVH builder over the bounded traced primitives.
//
// The reference has no acceleration structure: FrozenHittableList::hit tests
// every traced object in type order (hits.rs:274-285).  Its result is the
// smallest accepted root, ties going to the later object.  The BVH only decides
// WHICH exact tests run; boxes are conservative, and the kernel applies the same
// tie rule, so the closest hit is bit-identical to brute force.
#pragma once
#include "om_world.h"

namespace om {
void build_bvh(const om_world& w, FrozenWorld& fw, RefitTables* rt = nullptr);
// a sphere / ellipsoid whose test's error from OM_SPHERE_REACH away can pass its margin: outside every
// tree, no `culled` bound (§5.3)
bool thin_sphere(const Mat4& l2w);
// (the half-precision node planes, half_value and half_out, are in om_refit.h: the refit kernels round
// with them too)
}
