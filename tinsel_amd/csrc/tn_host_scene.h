// tn_host_scene.h -- the scene level (scene BVH, leaf boxes, plane table) derived and uploaded in one place; the C-ABI calls that edit it
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

// PrimitiveBounds (intersection.h:906-939) of primitive i as it is now: the local box (sphere: +-radius; plane: +-1e8; mesh: its root's)
// under the start and the end transform, TransformBounds (maths.h:1004-1021), united
void primitive_bounds(const tinsel_hip* r, int i, V3& lower, V3& upper)
{
    const Prim64& p = r->primsHost[(size_t)i];
    V3 lo, hi;
    if (p.type == kPrimSphere)      { lo = V3(-p.g0); hi = V3(p.g0); }
    else if (p.type == kPrimPlane)  { lo = V3(-1.e+8f); hi = V3(1.e+8f); }
    else                            { lo = r->meshRootLo[(size_t)r->primMesh[(size_t)i]]; hi = r->meshRootHi[(size_t)r->primMesh[(size_t)i]]; }
    V3 sl, su, el, eu;
    transform_bounds(r->primStart[(size_t)i], lo, hi, sl, su);
    transform_bounds(r->primEnd[(size_t)i], lo, hi, el, eu);
    lower = V3(minT(sl.x, el.x), minT(sl.y, el.y), minT(sl.z, el.z));      // Union, maths.h:1023-1026
    upper = V3(maxT(su.x, eu.x), maxT(su.y, eu.y), maxT(su.z, eu.z));
}

// a Node64 tree (as the device builders emit it) back into the reference's node array: what tinsel_hip_refit_mesh walks to refit
// the scene level, and what a later TINSEL_SCENE_BVH_NODES caller would hand in
void node64_to_reference(const std::vector<Node64>& nodes, uint32_t ref, float lminx, float lminy, float lminz, float lmaxx, float lmaxy, float lmaxz,
                         std::vector<tinsel_bvh_node>& out, uint32_t at)
{
    tinsel_bvh_node& me = out[at];
    me.lower.x = lminx; me.lower.y = lminy; me.lower.z = lminz;
    me.upper.x = lmaxx; me.upper.y = lmaxy; me.upper.z = lmaxz;
    if (ref & kLeafBit)
    {
        me.left_index = ref & ~kLeafBit;
        me.right_index_leaf = 0x80000000u;
        return;
    }
    const Node64 n = nodes[ref];
    const uint32_t l = (uint32_t)out.size();
    out.push_back(tinsel_bvh_node());
    out.push_back(tinsel_bvh_node());
    out[at].left_index = l;
    out[at].right_index_leaf = l + 1u;
    node64_to_reference(nodes, n.left, n.lminx, n.lminy, n.lminz, n.lmaxx, n.lmaxy, n.lmaxz, out, l);
    node64_to_reference(nodes, n.right, n.rminx, n.rminy, n.rminz, n.rmaxx, n.rmaxy, n.rmaxz, out, l + 1u);
}

// Every internal node of a reference-format tree becomes the union of its children's boxes, bottom-up: what the builder stores for that
// shape (min and max do not round).  Post-order from node 0; the tree must be acyclic (convert_bvh validated it).
void union_ancestors(std::vector<tinsel_bvh_node>& tree)
{
    std::vector<uint32_t> order, stack(1, 0u);
    while (!stack.empty())
    {
        const uint32_t k = stack.back();
        stack.pop_back();
        order.push_back(k);
        if (!ref_is_leaf(tree[k]))
        {
            stack.push_back(tree[k].left_index);
            stack.push_back(ref_right(tree[k]));
        }
    }
    for (size_t q = order.size(); q-- > 0; )
    {
        tinsel_bvh_node& n = tree[order[q]];
        if (ref_is_leaf(n))
            continue;
        const tinsel_bvh_node& a = tree[n.left_index];
        const tinsel_bvh_node& b = tree[ref_right(n)];
        n.lower.x = minT(a.lower.x, b.lower.x); n.lower.y = minT(a.lower.y, b.lower.y); n.lower.z = minT(a.lower.z, b.lower.z);
        n.upper.x = maxT(a.upper.x, b.upper.x); n.upper.y = maxT(a.upper.y, b.upper.y); n.upper.z = maxT(a.upper.z, b.upper.z);
    }
}

// The scene level: the device form of a scene BVH and what the flat scan derives from it.  A pure function of the tree, the primitives,
// the plane table and whether it may pair planes (build_scene_level): create, tinsel_hip_rebuild_scene and tinsel_hip_refit_mesh all go through it.
struct SceneLevel
{
    std::vector<tinsel_bvh_node> tree;  // in the reference's format (tinsel_hip::sceneBvhHost once in force)
    ConvertedBvh bvh;
    std::vector<PrimBox> boxes;         // by primitive: its leaf's box; 2 for a plane of the plane table
    std::vector<float> planeEq;         // DevScene::planeEq, four per slot, and DevScene::planeIdx: as many slots as create reserved, whatever is in them
    std::vector<int32_t> planeIdx;
    int32_t numPlanes = 0, planePairEnd = 0;    // DevScene's
    int planePairs = 0, planeSingles = 0;       // what the table holds (tinsel_hip_plane_table)
    unsigned long long scanMask = 0;    // DevScene::scanMask: the primitives < 64 the scan loop tests (those not in the plane table)
    bool everyPrimHasALeaf = true;
};

// May two planes of the plane table be tested as an OPPOSING PAIR (trace_flat, tn_plane.h)?  All eight coefficients finite, and each normal
// component of B the bitwise negation of A's, or both zeros of any sign -- what makes B's dot products the exact negations of A's.
bool plane_pair_ok(const float a[4], const float b[4])
{
    for (int c = 0; c < 4; ++c)
        if (!std::isfinite(a[c]) || !std::isfinite(b[c]))
            return false;
    for (int c = 0; c < 3; ++c)
    {
        uint32_t ua, ub;
        memcpy(&ua, &a[c], 4); memcpy(&ub, &b[c], 4);
        if (ub != (ua ^ 0x80000000u) && !(a[c] == 0.0f && b[c] == 0.0f))
            return false;
    }
    return true;
}

// The pairs among `eqs` (four floats per plane), greedily in order, no plane twice: (a, b) positions with a < b, by a
std::vector<std::pair<int, int>> pair_planes(const std::vector<float>& eqs)
{
    const int n = (int)(eqs.size()/4);
    std::vector<char> used((size_t)n, 0);
    std::vector<std::pair<int, int>> out;
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n && !used[(size_t)a]; ++b)
            if (!used[(size_t)b] && plane_pair_ok(&eqs[(size_t)a*4], &eqs[(size_t)b*4]))
            {
                used[(size_t)a] = used[(size_t)b] = 1;
                out.emplace_back(a, b);
            }
    return out;
}

// Slots of a plane table of `pairs` pairs and `singles` single planes: a block of eight per two pairs (A0 B0 A1 B1 R - - -: a single rides
// with them; an odd pair's block has no second pair), then the singles left, in fours (DevScene::planePairEnd)
int plane_table_slots(int pairs, int singles)
{
    const int blocks = (pairs + 1)/2, riders = std::min(blocks, singles);
    return 8*blocks + (singles - riders + 3)/4*4;
}

// The plane table (the flat scan's always-hit planes, tested ahead of the loop: opposing pairs with one division each, then the singles four
// at a time; plane_table_slots) on the level's boxes.  A table plane whose leaf box is no longer "infinite" (the primitive was scaled below 0.1, or the caller's
// tree has a tighter leaf) is box-tested in the loop like everything else and leaves the table -- a pair it was in dissolves, its partner is
// a single -- and one whose box is infinite again comes back (the table used to be written at create only).  Empty slots hold
// d == 0, IntersectRayPlane's own "no hit".  `pairPlanes` false (tinsel_hip_tuning::plane_pairs = 0): singles only.
void mark_plane_table(SceneLevel& lvl, const std::vector<Prim64>& prims, const std::vector<int32_t>& planeTable, bool pairPlanes)
{
    std::vector<int32_t> live;
    std::vector<float> eqs;
    for (const int32_t k : planeTable)
        if (lvl.boxes[(size_t)k].alwaysHit)
        {
            lvl.boxes[(size_t)k].alwaysHit = 2u;
            const Prim64& pp = prims[(size_t)k];
            live.push_back(k);
            eqs.insert(eqs.end(), { pp.g0, pp.g1, pp.g2, pp.g3 });
        }
    // What create reserved is what the table has, whatever moves later: room for every table plane as a single, and for the pairing of all of
    // them.  A later pairing that would take more (a pair dissolved, and its partner no longer fits a block of four) gives up pairs, last first.
    std::vector<float> all;
    for (const int32_t k : planeTable)
        all.insert(all.end(), { prims[(size_t)k].g0, prims[(size_t)k].g1, prims[(size_t)k].g2, prims[(size_t)k].g3 });
    const int allPairs = (int)pair_planes(all).size();
    const size_t cap = (size_t)std::max(plane_table_slots(0, (int)planeTable.size()), plane_table_slots(allPairs, (int)planeTable.size() - 2*allPairs));
    std::vector<std::pair<int, int>> pairs = pairPlanes ? pair_planes(eqs) : std::vector<std::pair<int, int>>();
    while ((size_t)plane_table_slots((int)pairs.size(), (int)live.size() - 2*(int)pairs.size()) > cap)
        pairs.pop_back();
    std::vector<char> paired(live.size(), 0);
    for (const auto& ab : pairs)
        paired[(size_t)ab.first] = paired[(size_t)ab.second] = 1;
    std::vector<int> singles;
    for (size_t t = 0; t < live.size(); ++t)
        if (!paired[t])
            singles.push_back((int)t);

    lvl.planeEq.assign(cap*4, 0.0f);
    lvl.planeIdx.assign(cap, 0);
    auto put = [&](size_t slot, int t) {
        std::copy(eqs.begin() + (size_t)t*4, eqs.begin() + (size_t)t*4 + 4, lvl.planeEq.begin() + slot*4);
        lvl.planeIdx[slot] = live[(size_t)t];
    };
    size_t slot = 0, nextSingle = 0;
    for (size_t q = 0; q < pairs.size(); q += 2, slot += 8)
    {
        put(slot, pairs[q].first); put(slot + 1, pairs[q].second);
        if (q + 1 < pairs.size())
        {
            put(slot + 2, pairs[q + 1].first); put(slot + 3, pairs[q + 1].second);
        }
        if (nextSingle < singles.size())
            put(slot + 4, singles[nextSingle++]);
        // (the four pair slots' indices once more, as the bytes of the first unused slot's word: trace_flat)
        lvl.planeIdx[slot + 5] = lvl.planeIdx[slot] | (lvl.planeIdx[slot + 1] << 8) | (lvl.planeIdx[slot + 2] << 16) | (lvl.planeIdx[slot + 3] << 24);
    }
    lvl.planePairEnd = (int32_t)slot;
    while (nextSingle < singles.size())
        put(slot++, singles[nextSingle++]);
    lvl.numPlanes = (int32_t)slot;
    lvl.planePairs = (int)pairs.size();
    lvl.planeSingles = (int)singles.size();

    lvl.scanMask = 0;
    for (size_t k = 0; k < lvl.boxes.size() && k < 64; ++k)
        if (lvl.boxes[k].alwaysHit != 2u)
            lvl.scanMask |= 1ull << k;
}

// Does the plane table of this renderer's scene pair its opposing planes under `tune`?
bool pairs_planes(const tinsel_hip* r, const tinsel_hip_tuning& tune) { return tune.plane_pairs != 0 && r->pairablePlanes; }

// The scene level of `tree` over `prims` (their count is what a leaf may index) and `planeTable`.  False, with nothing derived, where
// convert_bvh refuses the tree.
bool build_scene_level(std::vector<tinsel_bvh_node> tree, const std::vector<Prim64>& prims, const std::vector<int32_t>& planeTable, bool pairPlanes, SceneLevel& out)
{
    const int P = (int)prims.size();
    if (!convert_bvh(tree.data(), (int)tree.size(), P, 0, out.bvh))
        return false;
    // leaf boxes of the scene BVH, by primitive index (flat scene-level scan)
    out.boxes.assign((size_t)P, PrimBox());
    std::vector<char> seen((size_t)P, 0);
    for (const tinsel_bvh_node& nd : tree)
        if (ref_is_leaf(nd) && nd.left_index < (uint32_t)P)
        {
            out.boxes[nd.left_index] = make_prim_box(nd);
            seen[nd.left_index] = 1;
        }
    out.everyPrimHasALeaf = std::find(seen.begin(), seen.end(), 0) == seen.end();
    mark_plane_table(out, prims, planeTable, pairPlanes);
    out.tree = std::move(tree);
    return true;
}

// the host's half of a scene level in force (the launches take DevScene by value); create's arena holds the device's already
void adopt_scene_level(tinsel_hip* r, SceneLevel& lvl)
{
    r->scene.root = lvl.bvh.root;
    r->scene.scanMask = lvl.scanMask;
    r->scene.numPlanes = lvl.numPlanes;
    r->scene.planePairEnd = lvl.planePairEnd;
    r->planePairs = lvl.planePairs;
    r->planeSingles = lvl.planeSingles;
    r->sceneStackNeed = lvl.bvh.maxLeafDepth + 1;
    r->levelPlaneEq = lvl.planeEq;          // (what a baked instance is keyed by: tn_host_bake.h)
    r->levelPlaneIdx = lvl.planeIdx;
    r->levelBoxes = lvl.boxes;
    r->sceneBvhHost = std::move(lvl.tree);
}

// a scene level into the arena create laid out (its nodes, all P leaf boxes, the plane table's equations), then in force
int upload_scene_level(tinsel_hip* r, SceneLevel& lvl)
{
    unsigned char* arenaDev = const_cast<unsigned char*>(r->scene.arena);
    if (!lvl.bvh.nodes.empty())
        HIP_TRY(hipMemcpy(arenaDev + r->arenaOffNodes, lvl.bvh.nodes.data(), sizeof(Node64)*lvl.bvh.nodes.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(arenaDev + r->arenaOffBoxes, lvl.boxes.data(), sizeof(PrimBox)*lvl.boxes.size(), hipMemcpyHostToDevice));
    if (!lvl.planeEq.empty())
    {
        HIP_TRY(hipMemcpy(const_cast<float4*>(r->scene.planeEq), lvl.planeEq.data(), sizeof(float)*lvl.planeEq.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(const_cast<int32_t*>(r->scene.planeIdx), lvl.planeIdx.data(), sizeof(int32_t)*lvl.planeIdx.size(), hipMemcpyHostToDevice));
    }
    adopt_scene_level(r, lvl);
    return 0;
}

// the traversal stack a scene level `sceneNeed` deep over `meshes` takes, or -1 where it does not fit a workgroup's LDS beside the staged arena
int fitting_stack(const tinsel_hip* r, int sceneNeed, const std::vector<DevMesh>& meshes)
{
    int maxMeshNeed = 0;
    for (const DevMesh& dm : meshes)
        maxMeshNeed = std::max(maxMeshNeed, dm.stackNeed);
    const int stack = pick_stack(sceneNeed + maxMeshNeed);
    return stack >= 0 && stack_bytes(r, stack) <= (size_t)r->sharedMemLimit ? stack : -1;
}

// `build()` (device work on the null stream) between two events; when it succeeds, their span in milliseconds into *ms where given
// (tinsel_hip_set_mesh_bvh's is bench.py's mesh_bvh_build_ms)
template <class Build>
int timed_build(double* ms, Build&& build)
{
    Event e0, e1;
    if (e0.create(true) || e1.create(true))
        return -1;
    (void)hipEventRecord(e0, nullptr);
    const int rc = build();
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float t = 0.0f;
    (void)hipEventElapsedTime(&t, e0, e1);
    if (!rc && ms)
        *ms = t;
    return rc;
}

// PrimitiveArea of mesh primitive p as it is now, area*endTransform.s (intersection.h:843-847), and its reciprocal into p's Mat128 in the arena
int write_mesh_prim_area(tinsel_hip* r, int p)
{
    const float area = r->meshArea[(size_t)r->primMesh[(size_t)p]]*r->primEndScale[(size_t)p];
    const float rcpArea = 1.0f/area;
    unsigned char* mat = const_cast<unsigned char*>(r->scene.arena) + r->arenaOffMats + sizeof(Mat128)*(size_t)p;
    HIP_TRY(hipMemcpy(mat + offsetof(Mat128, area), &area, sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(mat + offsetof(Mat128, rcpArea), &rcpArea, sizeof(float), hipMemcpyHostToDevice));
    for (size_t l = 0; l < r->lightPrims.size() && l < r->lightMats.size(); ++l)        // (a baked instance states a light's 1/area: its key follows)
        if (r->lightPrims[l] == p)
        {
            r->lightMats[l].area = area;
            r->lightMats[l].rcpArea = rcpArea;
        }
    return 0;
}

} // namespace

extern "C" {

int tinsel_hip_set_mesh_bvh(tinsel_hip* r, int mode, double* build_ms)
{
    lookahead_cancel(r);
    if (!r || (mode != TINSEL_BVH_REFERENCE && mode != TINSEL_BVH_LBVH && mode != TINSEL_BVH_PLOC))
        return fail("set_mesh_bvh: bad arguments");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    if (build_ms)
        *build_ms = 0.0;

    std::vector<DevMesh> next = r->meshesRef;
    DevPool built;          // the new generation of trees: dropped on every failure below (a failed build's too), which keeps what was there
    const int rc = mode == TINSEL_BVH_REFERENCE ? 0 : timed_build(build_ms, [&] {
        int rc = 0;
        for (size_t m = 0; m < next.size() && !rc; ++m)
            if (!next[m].inArena && next[m].numTris >= 2)       // LDS-resident meshes keep their (tiny) reference trees
                rc = build_device_bvh(built, r->meshesRef[m], next[m], mode);
        return rc;
    });
    const int stack = rc ? -1 : fitting_stack(r, r->sceneStackNeed, next);
    if (stack < 0)
        return rc ? rc : fail("set_mesh_bvh: tree too deep for the LDS traversal stack (previous trees kept)");
    if (!next.empty())
        HIP_TRY(hipMemcpy((void*)r->scene.meshes, next.data(), sizeof(DevMesh)*next.size(), hipMemcpyHostToDevice));
    r->meshesNow = next;
    r->stackNeed = stack;
    r->bvhMode = mode;
    // the previous generation of device-built trees is unreachable now (a per-frame rebuild must not grow)
    r->lbvhTrees = std::move(built);
    return 0;
}

// Refit of a deforming mesh: new vertex positions (and optionally normals), same topology, same tree shape.
int tinsel_hip_refit_mesh(tinsel_hip* r, int primitive, const float* positions_xyz, int num_vertices, const float* normals_xyz)
{
    lookahead_cancel(r);
    if (!r || !positions_xyz || primitive < 0 || primitive >= r->scene.numPrims || r->primMesh[(size_t)primitive] < 0)
        return fail("refit_mesh: bad arguments (a mesh primitive and its new positions)");
    const int mi = r->primMesh[(size_t)primitive];
    DevMesh& dm = r->meshesNow[(size_t)mi];
    // (a mesh of the LDS-staged arena is refitted in the arena's copy in HBM, which every launch stages from)
    if (num_vertices != r->meshNumVertices[(size_t)mi])
        return fail("refit_mesh: the topology must not change (vertex count differs)");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());

    const int numTris = dm.numTris;
    const int numNodes = numTris - 1;           // one triangle per leaf: internal nodes
    {
        DevBuf<float> posDev, own;
        DevBuf<int> gen;
        if (posDev.upload(positions_xyz, 3*(size_t)num_vertices))
            return fail("refit_mesh: upload failed");
        hipLaunchKernelGGL(k_refit_tris, dim3((unsigned)((numTris + 255)/256)), dim3(256), 0, nullptr, const_cast<Tri48*>(dm.tris), numTris, posDev.get());
        if (normals_xyz && hipMemcpy(const_cast<float*>(dm.normals), normals_xyz, sizeof(float)*3*(size_t)num_vertices, hipMemcpyHostToDevice) != hipSuccess)
            return fail("refit_mesh: normals upload failed");
        if (numNodes > 0)
        {
            if (own.alloc(6*(size_t)numNodes) || gen.alloc((size_t)numNodes))
                return fail("refit_mesh: device allocation failed");
            // the tree in use and, when a device-built one is, the reference's too (switching back must not find stale boxes)
            const DevMesh* trees[2] = { &dm, r->meshesRef[(size_t)mi].nodes != dm.nodes ? &r->meshesRef[(size_t)mi] : nullptr };
            for (const DevMesh* tree : trees)
                if (tree && refit_device_bvh(*tree, dm.tris, own.get(), gen.get()))
                    return -1;
        }
        if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess)
            return fail("refit_mesh: kernels failed");
    }

    // Mesh::RebuildCDF (mesh.cpp:340-368) in the reference's own serial fp32 order, then PrimitiveArea of every instance
    const std::vector<int32_t>& idx = r->meshIndices[(size_t)mi];
    std::vector<float> cdf((size_t)numTris);
    float totalArea = 0.0f;
    for (int t = 0; t < numTris; ++t)
    {
        const float* a = positions_xyz + (size_t)idx[(size_t)t*3 + 0]*3;
        const float* b = positions_xyz + (size_t)idx[(size_t)t*3 + 1]*3;
        const float* c = positions_xyz + (size_t)idx[(size_t)t*3 + 2]*3;
        const V3 ab(b[0] - a[0], b[1] - a[1], b[2] - a[2]), ac(c[0] - a[0], c[1] - a[1], c[2] - a[2]);
        const float area = 0.5f*length(cross(ab, ac));
        totalArea += area;
        cdf[(size_t)t] = totalArea;
    }
    for (int t = 0; t < numTris; ++t)
        cdf[(size_t)t] /= totalArea;
    HIP_TRY(hipMemcpy(const_cast<float*>(dm.cdf), cdf.data(), sizeof(float)*(size_t)numTris, hipMemcpyHostToDevice));
    r->meshArea[(size_t)mi] = totalArea;
    for (int p = 0; p < r->scene.numPrims; ++p)
        if (r->primMesh[(size_t)p] == mi && write_mesh_prim_area(r, p))
            return -1;

    // The scene level follows: Scene::Build (scene.cpp:4-16) gives the scene BVH builder PrimitiveBounds(p) (intersection.h:906-939)
    // = the mesh root's box under the start and end transforms.  The tree keeps its shape here too: the leaf box of every
    // instance is recomputed with the reference's expressions and its ancestors become the union of their children.  Without this
    // a deformation that leaves the old box is clipped: the flat scan, the queue sort and k_walk's `enters` test all start from the
    // leaf box.
    V3 lo(kFltMax, kFltMax, kFltMax), hi(-kFltMax, -kFltMax, -kFltMax);     // the root's box: the union of the triangles' (Bounds::AddPoint)
    for (size_t k = 0; k < (size_t)numTris*3; ++k)
    {
        const float* v = positions_xyz + (size_t)idx[k]*3;
        lo = V3(minT(lo.x, v[0]), minT(lo.y, v[1]), minT(lo.z, v[2]));
        hi = V3(maxT(hi.x, v[0]), maxT(hi.y, v[1]), maxT(hi.z, v[2]));
    }
    r->meshRootLo[(size_t)mi] = lo;
    r->meshRootHi[(size_t)mi] = hi;
    std::vector<tinsel_bvh_node> tree = r->sceneBvhHost;
    for (tinsel_bvh_node& nd : tree)
        if (ref_is_leaf(nd) && nd.left_index < (uint32_t)r->scene.numPrims && r->primMesh[nd.left_index] == mi)
        {
            V3 l, u;
            primitive_bounds(r, (int)nd.left_index, l, u);
            nd.lower.x = l.x; nd.lower.y = l.y; nd.lower.z = l.z;
            nd.upper.x = u.x; nd.upper.y = u.y; nd.upper.z = u.z;
        }
    union_ancestors(tree);
    // (all P leaf boxes and the plane table are uploaded again: the other primitives' come from the same leaves as before, and a mesh is
    // never in the plane table)
    SceneLevel lvl;
    if (!build_scene_level(std::move(tree), r->primsHost, r->planeTablePrims, pairs_planes(r, r->tune), lvl))
        return fail("refit_mesh: the scene BVH could not be refitted");
    return upload_scene_level(r, lvl);
}

// A primitive moves (the reference mutates Scene::primitives[i].startTransform / endTransform and re-runs Scene::Build).
int tinsel_hip_set_primitive_transform(tinsel_hip* r, int index, const tinsel_transform* start, const tinsel_transform* end)
{
    lookahead_cancel(r);
    if (!r || !start || !end || index < 0 || index >= r->scene.numPrims)
        return fail("set_primitive_transform: bad arguments");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    const Xform xs = to_xform(*start), xe = to_xform(*end);
    const bool isStatic = memcmp(start, end, sizeof(tinsel_transform)) == 0;
    r->primStart[(size_t)index] = xs;
    r->primEnd[(size_t)index] = xe;
    r->primEndScale[(size_t)index] = xe.s;
    Prim64& o = r->primsHost[(size_t)index];
    set_prim_pose(o, xs, xe, isStatic);
    set_prim_derived(o);
    const Moving64 mv = make_moving(xs, xe);
    unsigned char* arenaDev = const_cast<unsigned char*>(r->scene.arena);
    HIP_TRY(hipMemcpy(arenaDev + r->arenaOffPrims + sizeof(Prim64)*(size_t)index, &o, sizeof(Prim64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(arenaDev + r->arenaOffMoving + sizeof(Moving64)*(size_t)index, &mv, sizeof(Moving64), hipMemcpyHostToDevice));
    if (o.type == kPrimMesh && write_mesh_prim_area(r, index))
        return -1;
    r->sceneDirty = true;
    return 0;
}

int tinsel_hip_rebuild_scene(tinsel_hip* r, int mode, const tinsel_bvh_node* nodes, int num_nodes, double* build_ms)
{
    lookahead_cancel(r);
    if (!r || (mode != TINSEL_SCENE_BVH_NODES && mode != TINSEL_SCENE_BVH_DEVICE) || (mode == TINSEL_SCENE_BVH_NODES && (!nodes || num_nodes <= 0)))
        return fail("rebuild_scene: bad arguments");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    if (build_ms)
        *build_ms = 0.0;
    const int P = r->scene.numPrims;

    std::vector<tinsel_bvh_node> ref;       // the new tree in the reference's format
    if (mode == TINSEL_SCENE_BVH_NODES)
        ref.assign(nodes, nodes + num_nodes);
    else
    {
        // leaf boxes: PrimitiveBounds of every primitive as it is now
        std::vector<V3> lo((size_t)P), hi((size_t)P);
        for (int i = 0; i < P; ++i)
            primitive_bounds(r, i, lo[(size_t)i], hi[(size_t)i]);
        ref.resize(1);
        if (P == 1)
            node64_to_reference({}, kLeafBit | 0u, lo[0].x, lo[0].y, lo[0].z, hi[0].x, hi[0].y, hi[0].z, ref, 0u);
        else
        {
            // The mesh builders' kernels over the primitives' boxes: a box travels as a degenerate triangle record (a = c = lower, b = upper),
            // whose min / max IS the box; Morton order of the centroids, agglomerative clustering by surface area (tn_lbvh.h)
            std::vector<Tri48> items((size_t)P);
            for (int i = 0; i < P; ++i)
            {
                Tri48& T = items[(size_t)i];
                T.ax = lo[(size_t)i].x; T.ay = lo[(size_t)i].y; T.az = lo[(size_t)i].z; T.i0 = i;
                T.bx = hi[(size_t)i].x; T.by = hi[(size_t)i].y; T.bz = hi[(size_t)i].z; T.i1 = i;
                T.cx = lo[(size_t)i].x; T.cy = lo[(size_t)i].y; T.cz = lo[(size_t)i].z; T.i2 = i;
            }
            DevBuf<Tri48> itemsDev;
            DevPool tree;               // the builder's own allocation for this tree: the arena takes a copy
            if (itemsDev.alloc((size_t)P))
                return -1;
            std::vector<Node64> built((size_t)P - 1);
            DevMesh fake, out;
            memset(&fake, 0, sizeof(fake));
            fake.tris = itemsDev.get();
            fake.numTris = P;
            fake.inArena = 1;           // (no bottom-level records for this one)
            if (hipMemcpy(itemsDev.get(), items.data(), sizeof(Tri48)*(size_t)P, hipMemcpyHostToDevice) != hipSuccess)
                return fail("rebuild_scene: upload failed");
            if (timed_build(build_ms, [&] { return build_device_bvh(tree, fake, out, TINSEL_BVH_PLOC); }))
                return -1;
            if (hipMemcpy(built.data(), out.nodes, sizeof(Node64)*((size_t)P - 1), hipMemcpyDeviceToHost) != hipSuccess)
                return fail("rebuild_scene: read-back failed");
            // root box: the union of its children's
            const Node64& rt = built[0];
            ref.reserve((size_t)2*P - 1);
            node64_to_reference(built, 0u, minT(rt.lminx, rt.rminx), minT(rt.lminy, rt.rminy), minT(rt.lminz, rt.rminz),
                                maxT(rt.lmaxx, rt.rmaxx), maxT(rt.lmaxy, rt.rmaxy), maxT(rt.lmaxz, rt.rmaxz), ref, 0u);
        }
    }

    // every check before anything is uploaded: a refused tree leaves the previous one in force
    SceneLevel lvl;
    if (!build_scene_level(std::move(ref), r->primsHost, r->planeTablePrims, pairs_planes(r, r->tune), lvl))
        return fail("rebuild_scene: malformed scene BVH");
    if ((int)lvl.bvh.nodes.size() != (P > 1 ? P - 1 : 0))
        return fail("rebuild_scene: the scene BVH must have one leaf per primitive");
    if (!lvl.everyPrimHasALeaf)
        return fail("rebuild_scene: a primitive has no leaf in the scene BVH");
    const int stack = fitting_stack(r, lvl.bvh.maxLeafDepth + 1, r->meshesNow);
    if (stack < 0)
        return fail("rebuild_scene: tree too deep for the LDS traversal stack (previous tree kept)");
    if (upload_scene_level(r, lvl))
        return -1;
    r->stackNeed = stack;
    r->sceneDirty = false;
    return 0;
}

} // extern "C"
