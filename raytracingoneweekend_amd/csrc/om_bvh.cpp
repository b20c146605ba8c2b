// om_bvh.cpp — binned-SAH BVH over spheres, cubes, triangles, parallelograms.
#include "om_bvh.h"
#include "om_tuning.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// SAH leaves: at most OM_BVH_MAX_LEAF records, always a leaf at OM_BVH_LEAF_FORCE or fewer; a tree
// whose compressed BVH2 does not fit the LDS budget (read through L2: S-10k) is rebuilt with the
// _L2 sizes: one record per leaf, so a ray reads fewer 64-B records and more 32-B half nodes (r05:
// C3 4258 / 4262 vs 4111 / 4119 Msamples/s at leaves <= 8, 4222 / 4240 at <= 2; C1, whose tree
// sits in LDS, 6558 / 6561 at 1 and 6950 / 7016 at 2 vs 7003 / 7016: profiles/r05_bvh2)
#ifndef OM_BVH_MAX_LEAF
#define OM_BVH_MAX_LEAF 8
#endif
#ifndef OM_BVH_LEAF_FORCE
#define OM_BVH_LEAF_FORCE 2
#endif
#ifndef OM_BVH_MAX_LEAF_L2
#define OM_BVH_MAX_LEAF_L2 1
#endif
#ifndef OM_BVH_LEAF_FORCE_L2
#define OM_BVH_LEAF_FORCE_L2 1
#endif
#ifndef OM_BVH_TRAV
#define OM_BVH_TRAV 1.0
#endif

namespace om {
namespace {

// (Box, inflate, bary_box and the outward f32 planes: om_refit.h, shared with the refit kernels)
struct Item { Box b; double c[3]; uint32_t gi; };

Box affine_box(const Mat4& l2w, double half) {
    Box b;
    for (int i = 0; i < 3; ++i) {
        const double a0 = l2w.r[i].e[0], a1 = l2w.r[i].e[1], a2 = l2w.r[i].e[2], c = l2w.r[i].e[3];
        // sphere (half < 0): exact ellipsoid extent = row norm; cube: 0.5 * L1 row norm
        const double h = half < 0 ? std::sqrt(a0 * a0 + a1 * a1 + a2 * a2) : half * (std::fabs(a0) + std::fabs(a1) + std::fabs(a2));
        b.lo[i] = c - h; b.hi[i] = c + h;
    }
    return inflate(b);
}

struct Builder {
    std::vector<Item> items;
    std::vector<OmBvhNode> nodes;
    std::vector<uint32_t> order;
    uint32_t max_leaf = OM_BVH_MAX_LEAF, leaf_force = OM_BVH_LEAF_FORCE;

    uint32_t emit(const Box& b) {
        OmBvhNode n;
        box_planes(b, n.lo, n.hi);
        n.left = 0; n.right = 0;
        nodes.push_back(n);
        return (uint32_t)(nodes.size() - 1);
    }

    // builds items[begin,end) ; returns node index
    // SAH down to depth kSahDepth, then median splits: depth <= kSahDepth + log2(n)
    // keeps every tree within the traversal stacks (kB2Stack entries, 64 for the global BVH).
    static constexpr uint32_t kSahDepth = 10;
    uint32_t build(uint32_t begin, uint32_t end, uint32_t depth = 0) {
        Box bb; bb.empty(); Box cb; cb.empty();
        for (uint32_t i = begin; i < end; ++i) { bb.grow(items[i].b); cb.grow_pt(items[i].c); }
        const uint32_t node = emit(bb);
        const uint32_t count = end - begin;
        auto make_leaf = [&]() {
            nodes[node].left = -(int32_t)(order.size() + 1);
            nodes[node].right = (int32_t)count;
            for (uint32_t i = begin; i < end; ++i) order.push_back(items[i].gi);
            return node;
        };
        if (count <= leaf_force) return make_leaf();
        // binned SAH over the centroid box
        const int NB = 16;
        double best_cost = 1e300; int best_axis = -1; int best_bin = -1;
        for (int ax = 0; ax < 3; ++ax) {
            const double lo = cb.lo[ax], hi = cb.hi[ax];
            if (!(hi - lo > 1e-12)) continue;
            Box bins[NB]; uint32_t cnt[NB] = {0};
            for (int k = 0; k < NB; ++k) bins[k].empty();
            for (uint32_t i = begin; i < end; ++i) {
                int k = (int)((items[i].c[ax] - lo) / (hi - lo) * NB);
                k = std::min(NB - 1, std::max(0, k));
                bins[k].grow(items[i].b); cnt[k]++;
            }
            Box lacc; lacc.empty(); uint32_t lc = 0;
            double la[NB]; uint32_t lcs[NB];
            for (int k = 0; k < NB - 1; ++k) { lacc.grow(bins[k]); lc += cnt[k]; la[k] = lacc.area(); lcs[k] = lc; }
            Box racc; racc.empty(); uint32_t rc = 0;
            for (int k = NB - 1; k > 0; --k) {
                racc.grow(bins[k]); rc += cnt[k];
                const uint32_t lcount = lcs[k - 1];
                if (lcount == 0 || rc == 0) continue;
                const double cost = la[k - 1] * lcount + racc.area() * rc;
                if (cost < best_cost) { best_cost = cost; best_axis = ax; best_bin = k; }
            }
        }
        const double leaf_cost = bb.area() * count;
        // traversal cost relative to one primitive test (OM_BVH_TRAV); leaves <= OM_BVH_MAX_LEAF (r01:
        // a sweep of cost 0.3-2 and max leaf 2-8 moved C1 by < 1%; r05 re-check in DESIGN.md §10)
        const double trav = OM_BVH_TRAV * bb.area();
        if (best_axis < 0 || depth >= kSahDepth) {
            if (count <= std::min(4u, max_leaf) || (best_axis < 0 && count <= 8)) return make_leaf();
            // degenerate centroids: median split on the longest box axis
            int ax = 0;
            for (int k = 1; k < 3; ++k) if (bb.hi[k] - bb.lo[k] > bb.hi[ax] - bb.lo[ax]) ax = k;
            std::nth_element(items.begin() + begin, items.begin() + begin + count / 2, items.begin() + end,
                             [ax](const Item& x, const Item& y) { return x.c[ax] < y.c[ax]; });
            const uint32_t mid = begin + count / 2;
            const uint32_t l = build(begin, mid, depth + 1);
            const uint32_t r = build(mid, end, depth + 1);
            nodes[node].left = (int32_t)l; nodes[node].right = (int32_t)r;
            return node;
        }
        if (count <= max_leaf && leaf_cost <= best_cost + trav) return make_leaf();
        const int ax = best_axis;
        const double lo = cb.lo[ax], hi = cb.hi[ax];
        auto mid_it = std::partition(items.begin() + begin, items.begin() + end, [&](const Item& it) {
            int k = (int)((it.c[ax] - lo) / (hi - lo) * NB);
            k = std::min(NB - 1, std::max(0, k));
            return k < best_bin;
        });
        uint32_t mid = (uint32_t)(mid_it - items.begin());
        if (mid == begin || mid == end) mid = begin + count / 2;
        const uint32_t l = build(begin, mid, depth + 1);
        const uint32_t r = build(mid, end, depth + 1);
        nodes[node].left = (int32_t)l; nodes[node].right = (int32_t)r;
        return node;
    }
};

}  // namespace


// Smallest and largest semi-axis of an ellipsoid: the extreme singular values of the 3x3 linear
// part (closed form for the eigenvalues of the symmetric A^T A, in double).
void semi_axes(const Mat4& l2w, double& rmin, double& rmax) {
    double s[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { s[i][j] = 0; for (int k = 0; k < 3; ++k) s[i][j] += (double)l2w.r[k].e[i] * (double)l2w.r[k].e[j]; }
    const double p1 = s[0][1] * s[0][1] + s[0][2] * s[0][2] + s[1][2] * s[1][2];
    const double q = (s[0][0] + s[1][1] + s[2][2]) / 3.0;
    const double p2 = (s[0][0] - q) * (s[0][0] - q) + (s[1][1] - q) * (s[1][1] - q) + (s[2][2] - q) * (s[2][2] - q) + 2.0 * p1;
    double lo = std::min(s[0][0], std::min(s[1][1], s[2][2])), hi = std::max(s[0][0], std::max(s[1][1], s[2][2]));
    if (p1 > 0.0 && p2 > 0.0) {
        const double p = std::sqrt(p2 / 6.0);
        double m[3][3];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) m[i][j] = (s[i][j] - (i == j ? q : 0.0)) / p;
        const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
        const double phi = std::acos(std::min(1.0, std::max(-1.0, 0.5 * det))) / 3.0;
        lo = q + 2.0 * p * std::cos(phi + 2.0943951023931953);
        hi = q + 2.0 * p * std::cos(phi);
    }
    rmin = std::sqrt(std::max(lo, 0.0)); rmax = std::sqrt(std::max(hi, 0.0));
}

// A sphere or ellipsoid stays outside every tree, and has no `culled` bound, when the error of its
// own test can pass its margin for a ray that starts OM_SPHERE_REACH away.  From the
// operation order of sphere_root, with u = 2^-24, L = |w2l (o - c)| <= D / rmin and a = |w2l d|^2:
// half_b = lo . ld carries 3u L sqrt(a), half_b^2 7u a L^2, c = lo . lo - 1 4u L^2, a 3u a, a c 8u a L^2,
// the subtraction u a L^2: disc / a is known to 16u L^2, so `disc >= 0` accepts a local distance from
// the centre of up to 1 + 8u L^2, which is at most 8u D^2 rmax / rmin^2 in the world.  (The roundings
// of lo and ld themselves only shift the ray, by a few u (C + D): the gradient of disc in lo is
// -2a times the perpendicular part of lo, of length 1 at the silhouette.)  The margin is the smallest
// the primitive gets: its box's, 1e-3 (1 + extent) + 1e-5 |coord| on the tightest axis, or its
// bounding sphere's, 1e-3 (1 + rmax) + 1e-5 |c|.  A non-finite transform compares false and stays.
bool thin_sphere(const Mat4& l2w) {
    double rmin, rmax;
    semi_axes(l2w, rmin, rmax);
    double h[3], mag = 0.0, cn = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double a0 = l2w.r[i].e[0], a1 = l2w.r[i].e[1], a2 = l2w.r[i].e[2], c = l2w.r[i].e[3];
        h[i] = std::sqrt(a0 * a0 + a1 * a1 + a2 * a2);
        mag = std::max(mag, std::max(std::fabs(c - h[i]), std::fabs(c + h[i])));
        cn += c * c;
    }
    double margin = 1e-3 * (1.0 + rmax) + 1e-5 * std::sqrt(cn);
    for (int i = 0; i < 3; ++i) margin = std::min(margin, 1e-3 * (1.0 + 2.0 * h[i]) + 1e-5 * mag);
    const double u = 5.9604644775390625e-8, D = OM_SPHERE_REACH;
    return 8.0 * u * D * D * rmax / (rmin * rmin) > margin;
}

// The builder in stages, each with one output; build_bvh at the end of the file runs them in order on
// the fresh FrozenWorld that freeze hands it.
namespace {

// Stage 1, select: every traced primitive once, as an item of the SAH builder or as a record tested
// outside the trees (`always`, ascending gi: the kinds are visited in gi order) with its conservative
// box, infinite when unbounded.  Outside go the planes, a bound above kHuge and a thin sphere (all
// unbounded: a huge sphere's inflation would cover the scene).  leaf_trees = false selects for the
// global BVH, which takes every triangle and parallelogram.  leaf_trees = true selects for the
// leaf-record trees (SBVH / BVH2 / BVH4): from OM_BARY_TREE_MIN of them on (§5.17), the
// triangles and parallelograms with a finite frozen record and a finite box are items beside the
// spheres and cubes (a huge one outside with its box); one with a non-finite value is outside and
// unbounded, so no cull ever sees a NaN.  Below the threshold every one of them is outside with its
// bary_box, the layout of every world before meshes.
struct Selection { std::vector<Item> items; std::vector<OmAlwaysRec> always; };

Selection select(const om_world& w, const FrozenWorld& fw, bool leaf_trees) {
    Selection s;
    const double kHuge = 100.0;  // a bound larger than this is tested outside the trees
    auto outside = [&](uint32_t gi, const Box* box) {
        OmAlwaysRec r;
        r.gi = gi; r.pad = 0;
        if (gi < fw.offsets[K_SPHERE + 1]) {      // axis-aligned sphere: every off-diagonal entry of W2L is +-0
            const float* m = fw.sph_test[gi - fw.offsets[K_SPHERE]].w2l;
            if (m[1] == 0.0f && m[2] == 0.0f && m[4] == 0.0f && m[6] == 0.0f && m[8] == 0.0f && m[9] == 0.0f)
                r.pad = OM_ALWAYS_DIAG_SPHERE;
        }
        if (box) box_planes(*box, r.lo, r.hi);
        else for (int i = 0; i < 3; ++i) { r.lo[i] = -INFINITY; r.hi[i] = INFINITY; }
        s.always.push_back(r);
    };
    auto add = [&](const Box& box, uint32_t gi, bool thin, bool boxed_outside) {
        double ext = 0.0;
        for (int i = 0; i < 3; ++i) ext = std::max(ext, box.hi[i] - box.lo[i]);
        if (ext > 2.0 * kHuge || thin) { outside(gi, boxed_outside ? &box : nullptr); return; }
        Item it; it.b = box; it.gi = gi;
        for (int i = 0; i < 3; ++i) it.c[i] = 0.5 * (box.lo[i] + box.hi[i]);
        s.items.push_back(it);
    };
    size_t n_bary_ok = 0;
    struct Bary { std::vector<Box> box; std::vector<uint8_t> ok; };
    auto measure = [&](const std::vector<BaryPrim>& prims, const std::vector<OmBary>& recs, bool para) {
        Bary b;
        for (size_t i = 0; i < prims.size(); ++i) {
            const Box bx = bary_box(prims[i], para);
            const float* f = (const float*)&recs[i];
            bool ok = true;
            for (size_t k = 0; k < sizeof(OmBary) / 4u; ++k) ok = ok && std::isfinite(f[k]);
            for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(bx.lo[k]) && std::isfinite(bx.hi[k]);
            b.box.push_back(bx); b.ok.push_back(ok);
            n_bary_ok += ok;
        }
        return b;
    };
    const Bary tri = measure(w.triangles, fw.tri, false), para = measure(w.parallelograms, fw.para, true);
    const bool bary_tree = n_bary_ok >= (size_t)OM_BARY_TREE_MIN;
    auto add_bary = [&](const Bary& b, uint32_t gi0) {
        for (size_t i = 0; i < b.box.size(); ++i) {
            if (!leaf_trees || (bary_tree && b.ok[i])) add(b.box[i], gi0 + (uint32_t)i, false, true);
            else outside(gi0 + (uint32_t)i, bary_tree ? nullptr : &b.box[i]);
        }
    };
    for (size_t i = 0; i < w.spheres.size(); ++i) add(affine_box(w.spheres[i].l2w, -1.0), fw.offsets[K_SPHERE] + (uint32_t)i, thin_sphere(w.spheres[i].l2w), false);
    for (size_t i = 0; i < w.cubes.size(); ++i) add(affine_box(w.cubes[i].l2w, 0.5), fw.offsets[K_CUBE] + (uint32_t)i, false, false);
    add_bary(tri, fw.offsets[K_TRI]);
    for (size_t i = 0; i < w.planes.size(); ++i) outside(fw.offsets[K_PLANE] + (uint32_t)i, nullptr);
    add_bary(para, fw.offsets[K_PARA]);
    return s;
}

// Stage 2, build: the SAH tree over the items (the root is node 0) with its stats, from the builder's
// own nodes: internal nodes, leaves, internal nodes on the deepest root-to-leaf path (the compressed
// tree's lane-stack bound) and the records of the largest leaf.
struct Tree {
    std::vector<OmBvhNode> nodes;
    std::vector<uint32_t> order;
    size_t internal = 0, leaves = 0;
    uint32_t depth = 0, max_leaf = 0;
};

Tree sah_tree(Builder& b, uint32_t max_leaf, uint32_t leaf_force) {
    Tree t;
    b.max_leaf = max_leaf; b.leaf_force = leaf_force;
    b.build(0, (uint32_t)b.items.size());
    t.nodes.swap(b.nodes); t.order.swap(b.order);
    std::vector<uint32_t> d(t.nodes.size(), 1u);             // parents precede children
    for (size_t n = 0; n < t.nodes.size(); ++n) {
        const OmBvhNode& nd = t.nodes[n];
        if (nd.left < 0) { ++t.leaves; t.max_leaf = std::max(t.max_leaf, (uint32_t)nd.right); continue; }
        ++t.internal; t.depth = std::max(t.depth, d[n]);
        d[(uint32_t)nd.left] = d[(uint32_t)nd.right] = d[n] + 1u;
    }
    return t;
}

// The tree of the leaf records.  One whose BVH2 is read through L2 (past kB2LdsBudget) is rebuilt with
// the _L2 leaf sizes.  One record per leaf gives one leaf per bounded primitive, which breaks the
// 16-bit codes and the lane stack (om::plan_trees' b2_ok) from ~32k primitives on: the max-leaf tree
// is kept then.
Tree build_tree(std::vector<Item> items) {
    Builder b;
    b.items = std::move(items);
    Tree t = sah_tree(b, OM_BVH_MAX_LEAF, OM_BVH_LEAF_FORCE);
    if (t.internal * sizeof(OmBvh2Node) + t.leaves * 4u > kB2LdsBudget) {
        Tree l2 = sah_tree(b, OM_BVH_MAX_LEAF_L2, OM_BVH_LEAF_FORCE_L2);
        if (l2.internal < kCode16Limit && l2.leaves < kCode16Limit && l2.depth <= kB2Stack) return l2;
    }
    return t;
}

// The global BVH over every bounded traced primitive: bvh, bvh_prims, always.
void build_global(const om_world& w, FrozenWorld& fw, Selection& s, bool keep) {
    Builder b;
    s = select(w, fw, false);
    for (const OmAlwaysRec& r : s.always) fw.always.push_back(r.gi);
    if (keep) b.items = s.items; else b.items.swap(s.items);     // keep: the refit tables read the selection afterwards
    if (b.items.empty()) return;
    Tree t = sah_tree(b, OM_BVH_MAX_LEAF, OM_BVH_LEAF_FORCE);
    fw.bvh.swap(t.nodes);
    fw.bvh_prims.swap(t.order);
}

// Stage 3, the stackless layout: the tree re-emitted in depth-first order with a skip
// ("miss") link per node (snodes), and the primitives' test records copied in leaf order so a leaf
// owns a contiguous run (srecs, n_srec_bary).  -> per builder node, the first record of a leaf
std::vector<uint32_t> emit_skip(const Tree& t, FrozenWorld& fw, std::vector<uint32_t>* src) {
    std::vector<uint32_t> leaf_first(t.nodes.size(), 0);
    struct Emit {
        const Tree& t; FrozenWorld& fw; std::vector<uint32_t>& leaf_first; std::vector<uint32_t>* src;
        void rec(uint32_t n) {
            if (src) src->push_back(n);
            const OmBvhNode& src = t.nodes[n];
            const uint32_t idx = (uint32_t)fw.snodes.size();
            OmSkipNode o;
            for (int i = 0; i < 3; ++i) { o.lo[i] = src.lo[i]; o.hi[i] = src.hi[i]; }
            o.skip = 0; o.leaf = 0xFFFFFFFFu;
            fw.snodes.push_back(o);
            if (src.left < 0) {
                const uint32_t first = (uint32_t)(-src.left - 1), cnt = (uint32_t)src.right;
                fw.snodes[idx].leaf = ((uint32_t)fw.srecs.size() << 8) | cnt;
                leaf_first[n] = (uint32_t)fw.srecs.size();
                for (uint32_t k = 0; k < cnt; ++k) {
                    const uint32_t gi = t.order[first + k];
                    const bool bary = gi >= fw.offsets[K_TRI];       // a slot with only its tag (om_layout.h)
                    const bool cube = !bary && gi >= fw.offsets[K_CUBE];
                    OmAffineTest r = bary ? OmAffineTest{} : cube ? fw.cube_test[gi - fw.offsets[K_CUBE]] : fw.sph_test[gi];
                    const uint32_t tag = gi | (cube ? OM_REC_CUBE : 0u) | (bary ? OM_REC_BARY : 0u);
                    std::memcpy(&r.pad, &tag, 4);
                    fw.srecs.push_back(r);
                    fw.n_srec_bary += bary ? 1u : 0u;
                }
            } else {
                rec((uint32_t)src.left);
                rec((uint32_t)src.right);
            }
            fw.snodes[idx].skip = (uint32_t)fw.snodes.size();
        }
    } e{t, fw, leaf_first, src};
    e.rec(0u);
    return leaf_first;
}

// Stage 4, the compressed BVH2: both child boxes in the parent (one read per visit), emitted
// breadth-first so the top levels, which every ray visits, are the first nodes: a tree too big for LDS
// stages that prefix there (om_wavefront.hip, OM_WF_HYB_BYTES).  One walk for both forms: `box` stores
// child k's box in a node, `leaf` makes the code of a leaf child from its (first record, count).  A
// single leaf becomes one node whose second child is an empty leaf.
template <class Node, class BoxFn, class LeafFn>
void emit_bvh2(const Tree& t, const std::vector<uint32_t>& leaf_first, std::vector<Node>& out, BoxFn box, LeafFn leaf,
               std::vector<uint32_t>* box_src = nullptr) {
    OmBvhNode none{};
    for (int i = 0; i < 3; ++i) { none.lo[i] = INFINITY; none.hi[i] = -INFINITY; }
    const bool one = t.nodes[0].left < 0;
    std::vector<std::pair<uint32_t, uint32_t>> q{{0u, 0u}};   // (builder node, output index)
    out.assign(1, Node{});
    auto code = [&](uint32_t c) {
        if (t.nodes[c].left < 0) return leaf(leaf_first[c], (uint32_t)t.nodes[c].right);
        out.push_back(Node{});
        q.emplace_back(c, (uint32_t)(out.size() - 1));
        return (uint32_t)(out.size() - 1);
    };
    for (size_t h = 0; h < q.size(); ++h) {
        const OmBvhNode& src = t.nodes[q[h].first];
        Node o{};
        box(o, 0, one ? src : t.nodes[(uint32_t)src.left]);
        box(o, 1, one ? none : t.nodes[(uint32_t)src.right]);
        o.c0 = code(one ? 0u : (uint32_t)src.left);
        o.c1 = one ? leaf(0u, 0u) : code((uint32_t)src.right);
        out[q[h].second] = o;
        if (box_src) {                                        // per output node: the builder nodes of its two boxes
            if (box_src->size() < 2u * out.size()) box_src->resize(2u * out.size(), kRefitNoNode);
            (*box_src)[2u * q[h].second] = one ? 0u : (uint32_t)t.nodes[q[h].first].left;
            (*box_src)[2u * q[h].second + 1u] = one ? kRefitNoNode : (uint32_t)t.nodes[q[h].first].right;
        }
    }
}

// The f32 form with 16-bit codes and its leaf table (b2nodes, b2leaves, b2_direct).  Direct leaf codes:
// when every record index fits kDirectFirst16 and every leaf holds at most kLeafCountMax records
// (S-traced: 482 records, leaves <= 2; every regime: DESIGN.md §5.6), a leaf child's code is
// OM_LEAF | first << 4 | count, so the traversal needs no leaf-table read to enter a leaf; the table
// is still emitted (same order) for the other consumers.  (Both conditions checked here, not assumed
// from the builder's leaf cap: a larger count would spill into the `first` bits)
void emit_b2(const Tree& t, const std::vector<uint32_t>& leaf_first, FrozenWorld& fw, std::vector<uint32_t>* src) {
    const bool direct = fw.srecs.size() < kDirectFirst16 && t.max_leaf <= kLeafCountMax;
    fw.b2_direct = direct ? 1u : 0u;
    emit_bvh2(t, leaf_first, fw.b2nodes,
              [](OmBvh2Node& o, int k, const OmBvhNode& c) {
                  for (int i = 0; i < 3; ++i) { (k ? o.lo1 : o.lo0)[i] = c.lo[i]; (k ? o.hi1 : o.hi0)[i] = c.hi[i]; }
              },
              [&](uint32_t first, uint32_t cnt) {
                  fw.b2leaves.push_back((first << 8) | cnt);
                  return OM_LEAF | (direct ? (first << kLeafCountBits) | cnt : (uint32_t)(fw.b2leaves.size() - 1));
              }, src);
}

// The half-precision copy of b2nodes (b2h).
void emit_b2h(FrozenWorld& fw) {
    for (const OmBvh2Node& n : fw.b2nodes) {
        OmBvh2NodeH h{};
        for (int i = 0; i < 3; ++i) {
            h.b[i] = half_out(OM_B2_LO(n, 0, i), false); h.b[3 + i] = half_out(OM_B2_HI(n, 0, i), true);
            h.b[6 + i] = half_out(OM_B2_LO(n, 1, i), false); h.b[9 + i] = half_out(OM_B2_HI(n, 1, i), true);
        }
        h.c0 = (uint16_t)n.c0; h.c1 = (uint16_t)n.c1; h.pad = 0u;
        fw.b2h.push_back(h);
    }
}

// The wide form (b2w; OmBvh2NodeW): the same tree in the same order with half planes
// and direct 32-bit codes, for every world whose records fit the leaf code (the 16-bit codes collide
// from index kCode16Limit on, so nothing here reads b2nodes / b2h / b2leaves).
void emit_b2w(const Tree& t, const std::vector<uint32_t>& leaf_first, FrozenWorld& fw) {
    if (!(fw.srecs.size() < kDirectFirst32 && t.max_leaf <= kLeafCountMax)) return;
    emit_bvh2(t, leaf_first, fw.b2w,
              [](OmBvh2NodeW& o, int k, const OmBvhNode& c) {
                  for (int i = 0; i < 3; ++i) { o.b[6 * k + i] = half_out(c.lo[i], false); o.b[6 * k + 3 + i] = half_out(c.hi[i], true); }
              },
              [](uint32_t first, uint32_t cnt) { return OM_LEAFW | (first << kLeafCountBits) | cnt; });
}

// Stage 5: the conservative world box of every leaf record (srec_box; the tree's own item boxes).
void emit_srec_box(const om_world& w, FrozenWorld& fw) {
    for (const OmAffineTest& t : fw.srecs) {
        uint32_t tag;
        std::memcpy(&tag, &t.pad, 4);
        const uint32_t gi = tag & OM_REC_GI;
        const Box bx = (tag & OM_REC_BARY) ? (gi >= fw.offsets[K_PARA] ? bary_box(w.parallelograms[gi - fw.offsets[K_PARA]], true)
                                                                       : bary_box(w.triangles[gi - fw.offsets[K_TRI]], false))
                     : (tag & OM_REC_CUBE) ? affine_box(w.cubes[gi - fw.offsets[K_CUBE]].l2w, 0.5)
                                           : affine_box(w.spheres[gi].l2w, -1.0);
        float p[6];
        box_planes(bx, p, p + 3);
        fw.srec_box.insert(fw.srec_box.end(), p, p + 6);
    }
}

// Stage 6, the BVH4 (b4nodes, b4h, b4_depth): each wide node takes its BVH2 node's two
// children and keeps replacing the internal child of largest surface area by that child's two children,
// up to four.  Child boxes are the BVH2's (already conservative), so culling stays exact.  Collapsed
// from the 16-bit codes of b2nodes: none for a tree past them.
void build_bvh4(FrozenWorld& fw, RefitTables* rt) {
    if (fw.b2nodes.empty() || fw.b2nodes.size() >= kCode16Limit || fw.b2leaves.size() >= kCode16Limit) return;
    struct Ch { uint32_t code; float lo[3], hi[3]; uint32_t src; };      // src: the builder node of the box (refit)
    auto kids = [&](uint32_t n, Ch* out) {
        const OmBvh2Node& N = fw.b2nodes[n];
        out[0].code = N.c0; out[1].code = N.c1;
        out[0].src = rt ? rt->b2_src[2u * n] : kRefitNoNode; out[1].src = rt ? rt->b2_src[2u * n + 1u] : kRefitNoNode;
        for (int i = 0; i < 3; ++i) {
            out[0].lo[i] = OM_B2_LO(N, 0, i); out[0].hi[i] = OM_B2_HI(N, 0, i);
            out[1].lo[i] = OM_B2_LO(N, 1, i); out[1].hi[i] = OM_B2_HI(N, 1, i);
        }
    };
    auto area = [](const Ch& c) {
        const double dx = std::max(0.0, (double)c.hi[0] - c.lo[0]), dy = std::max(0.0, (double)c.hi[1] - c.lo[1]),
                     dz = std::max(0.0, (double)c.hi[2] - c.lo[2]);
        return dx * dy + dy * dz + dz * dx;
    };
    struct Rec {
        FrozenWorld& fw; decltype(kids)& kids_of; decltype(area)& area_of; RefitTables* rt;
        uint32_t go(uint32_t n2, uint32_t depth) {
            std::vector<Ch> ch(2);
            kids_of(n2, ch.data());
            while (ch.size() < 4) {
                int best = -1; double ba = -1.0;
                for (size_t i = 0; i < ch.size(); ++i)
                    if (!(ch[i].code & OM_LEAF) && area_of(ch[i]) > ba) { ba = area_of(ch[i]); best = (int)i; }
                if (best < 0) break;
                Ch two[2];
                kids_of(ch[best].code, two);
                ch[best] = two[0];
                ch.insert(ch.begin() + best + 1, two[1]);
            }
            const uint32_t idx = (uint32_t)fw.b4nodes.size();
            fw.b4nodes.push_back(OmBvh4Node{});
            fw.b4_depth = std::max(fw.b4_depth, depth);
            OmBvh4Node o{};
            for (int k = 0; k < 4; ++k) {
                if (k < (int)ch.size()) {
                    o.lox[k] = ch[k].lo[0]; o.loy[k] = ch[k].lo[1]; o.loz[k] = ch[k].lo[2];
                    o.hix[k] = ch[k].hi[0]; o.hiy[k] = ch[k].hi[1]; o.hiz[k] = ch[k].hi[2];
                    o.child[k] = (uint16_t)((ch[k].code & OM_LEAF) ? ch[k].code : go(ch[k].code, depth + 1));
                } else {
                    o.lox[k] = o.loy[k] = o.loz[k] = o.hix[k] = o.hiy[k] = o.hiz[k] = 0.0f;
                    o.child[k] = (uint16_t)OM_EMPTY;
                }
            }
            fw.b4nodes[idx] = o;
            if (rt) {
                if (rt->b4_src.size() < 4u * fw.b4nodes.size()) rt->b4_src.resize(4u * fw.b4nodes.size(), kRefitNoNode);
                for (size_t k = 0; k < ch.size(); ++k) rt->b4_src[4u * idx + k] = ch[k].src;
            }
            return idx;
        }
    } r{fw, kids, area, rt};
    r.go(0, 1);
    // breadth-first renumbering with half-precision planes (trees read through L2, §5.7)
    std::vector<uint32_t> order{0u}, pos(fw.b4nodes.size(), 0u);
    for (size_t h = 0; h < order.size(); ++h)
        for (uint16_t c : fw.b4nodes[order[h]].child)
            if (c != OM_EMPTY && !(c & OM_LEAF)) { pos[c] = (uint32_t)order.size(); order.push_back(c); }
    for (uint32_t n : order) {
        const OmBvh4Node& N = fw.b4nodes[n];
        OmBvh4NodeH o{};
        for (int k = 0; k < 4; ++k) {
            o.b[k] = half_out(N.lox[k], false); o.b[4 + k] = half_out(N.loy[k], false); o.b[8 + k] = half_out(N.loz[k], false);
            o.b[12 + k] = half_out(N.hix[k], true); o.b[16 + k] = half_out(N.hiy[k], true); o.b[20 + k] = half_out(N.hiz[k], true);
            const uint16_t c = N.child[k];
            o.child[k] = (c == OM_EMPTY || (c & OM_LEAF)) ? c : (uint16_t)pos[c];
        }
        fw.b4h.push_back(o);
        if (rt) rt->b4h_src.insert(rt->b4h_src.end(), rt->b4_src.begin() + 4u * n, rt->b4_src.begin() + 4u * n + 4u);
    }
}

// What a refit of the uploaded world needs (om_refit.h), from the stages' own data: the box of every
// primitive that is an item of a tree or a boxed record outside, the two topologies by depth, and
// per stored box of every layout its builder node (the src arrays the stages filled).
void keep_for_refit(const FrozenWorld& fw, const Selection& global, const Selection& leaf, const Tree* t,
                    const std::vector<uint32_t>& leaf_first, RefitTables& rt) {
    const uint32_t n_traced = fw.offsets[K_MSPHERE];
    rt.covering = n_traced;
    rt.tri_first = fw.offsets[K_TRI];
    rt.prim_box.resize(6u * ((size_t)n_traced + 1u));
    for (uint32_t gi = 0; gi < n_traced; ++gi) box_none(&rt.prim_box[6u * (size_t)gi]);
    box_covering(&rt.prim_box[6u * (size_t)n_traced]);
    auto keep = [&](uint32_t gi, const float* lo, const float* hi) {
        bool ok = true;
        for (int i = 0; i < 3; ++i) ok = ok && finite_f32(lo[i]) && finite_f32(hi[i]);
        if (!ok) return;                     // unbounded outside, or an item the unions' min / max skip
        for (int i = 0; i < 3; ++i) { rt.prim_box[6u * (size_t)gi + i] = lo[i]; rt.prim_box[6u * (size_t)gi + 3 + i] = hi[i]; }
    };
    for (const Selection* s : {&global, &leaf}) {
        for (const Item& it : s->items) { float p[6]; box_planes(it.b, p, p + 3); keep(it.gi, p, p + 3); }
        for (const OmAlwaysRec& r : s->always) keep(r.gi, r.lo, r.hi);
    }
    refit_levels(fw.bvh, rt.g_level, rt.g_level_off);
    rt.tri_rec.assign(fw.counts[K_TRI], kRefitNoNode);
    if (!t) return;
    rt.tnodes = t->nodes;
    for (size_t n = 0; n < rt.tnodes.size(); ++n)
        if (rt.tnodes[n].left < 0) rt.tnodes[n].left = -(int32_t)(leaf_first[n] + 1u);      // items: the leaf's records
    for (size_t r = 0; r < fw.srecs.size(); ++r) {
        uint32_t tag;
        std::memcpy(&tag, &fw.srecs[r].pad, 4);
        const uint32_t gi = tag & OM_REC_GI;
        rt.titems.push_back(gi);
        if (gi >= fw.offsets[K_TRI] && gi < fw.offsets[K_TRI + 1]) rt.tri_rec[gi - fw.offsets[K_TRI]] = (uint32_t)r;
    }
    refit_levels(rt.tnodes, rt.t_level, rt.t_level_off);
}

}  // namespace

void build_bvh(const om_world& w, FrozenWorld& fw, RefitTables* rt) {
    if (rt) *rt = RefitTables();
    if (w.triangles.empty()) rt = nullptr;          // nothing can move
    Selection g;
    build_global(w, fw, g, rt != nullptr);
    Selection s = select(w, fw, true);
    for (const OmAlwaysRec& r : s.always) fw.always2.push_back(r.gi);
    if (rt) fw.always2_rec = s.always; else fw.always2_rec.swap(s.always);
    if (s.items.empty()) {
        if (rt) keep_for_refit(fw, g, s, nullptr, {}, *rt);
        return;
    }
    const Tree t = rt ? build_tree(s.items) : build_tree(std::move(s.items));
    const std::vector<uint32_t> leaf_first = emit_skip(t, fw, rt ? &rt->snode_src : nullptr);
    emit_b2(t, leaf_first, fw, rt ? &rt->b2_src : nullptr);
    emit_b2h(fw);
    emit_b2w(t, leaf_first, fw);
    // the traversals' stack bounds: a single leaf still takes one node
    fw.b2_depth = std::max(t.depth, 1u);
    fw.b2w_depth = fw.b2w.empty() ? 0u : fw.b2_depth;
    fw.b2_max_leaf = t.max_leaf;
    emit_srec_box(w, fw);
    build_bvh4(fw, rt);
    if (rt) keep_for_refit(fw, g, s, &t, leaf_first, *rt);
}

}  // namespace om
