// om_refit_dev.h — the device side of om_update_triangles (om_refit.hip), as the C API
// (om_render.hip) drives it: the refit tables of an uploaded world and one update on a stream.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "om_layout.h"
#include "om_refit.h"

namespace omr {

// om::RefitTables on the device.  The arrays of the world itself (records, nodes
// of every layout) are the scene's; these are what the emission stages knew beside them.
struct Tables {
    float* prim_box = nullptr;           // 6 per traced primitive by gi, then the covering box
    uint32_t n_prim = 0, covering = 0;   // boxes in prim_box; the index of the covering one
    uint32_t tri_first = 0, n_tri = 0;   // gi of triangle 0; triangles
    uint32_t* tri_rec = nullptr;         // per triangle: its record of srecs or kRefitNoNode
    uint32_t* g_level = nullptr;         // the global BVH's internal nodes by depth
    std::vector<uint32_t> g_level_off;
    OmBvhNode* tnodes = nullptr;         // the leaf-record tree
    uint32_t n_tnodes = 0;
    uint32_t* titems = nullptr;          // per record: its box among prim_box
    uint32_t n_titems = 0;
    uint32_t* t_level = nullptr;
    std::vector<uint32_t> t_level_off;
    uint32_t *snode_src = nullptr, *b2_src = nullptr, *b4_src = nullptr, *b4h_src = nullptr;
    uint32_t n_snode = 0, n_b2 = 0, n_b2h = 0, n_b2w = 0, n_b4 = 0;   // nodes of each layout the device holds
    uint32_t* info = nullptr;            // kInfoWords words of the last update
    bool ready() const { return prim_box != nullptr; }
};
enum { kInfoUnbounded = 0, kInfoSkipped = 1, kInfoWords = 2 };

// One update, asynchronous on `stream`: the records and boxes of triangles [first, first + n_tri)
// from dev_vertices (dev_indices null: vertices 3k, 3k + 1, 3k + 2), every internal box bottom-up,
// one launch per tree level, then the planes of every layout.  S: the scene whose arrays are rewritten.
hipError_t update(const Tables& t, const OmSceneDev& S, uint32_t first, const float* dev_vertices, uint32_t n_vertices,
                  const uint32_t* dev_indices, uint32_t n_tri, hipStream_t stream);

}  // namespace omr
