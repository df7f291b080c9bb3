// tn_host_create.h -- C-ABI: last_error, create (scene flattening + upload), destroy
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

void comm_release(tinsel_hip* r);       // (tn_host_group.h: the RCCL communicator of the process-per-GPU arm)

// ---------------------------------------------------------------------------
// tinsel_hip_create_tuned as steps.  What the steps hand to each other is SceneBuild; each step reports through fail() and returns early,
// and the renderer under construction frees whatever it holds when one does (std::unique_ptr in tinsel_hip_create_tuned).  The order of
// every arena.add and of every upload is part of the format: arena offsets are visible to kernels and to tinsel_hip_mesh_tree.

struct SceneBuild
{
    tinsel_hip* r;                  // the renderer under construction
    DevScene& sc;                   // its r->scene
    const tinsel_scene_desc* desc;
    const tinsel_hip_tuning& tune;
    int P;
    std::vector<Prim64> prims;
    std::vector<Mat128> mats;
    std::vector<Moving64> moving;
    std::vector<DevMesh> meshes;
    std::vector<int32_t> lights;
    std::map<uint64_t, uint32_t> meshIndex;     // MeshGeometry::id (util.h:20) -> DevScene::meshes index
    ArenaBuilder arena;
    int maxMeshNeed = 0;
    int totalLightSamples = 0;
    bool sceneHasBigMesh = false;
    SceneLevel lvl;
    bool flatScan = false;
    // DRY: the host's half only -- every record, offset, flag and count as create derives them, nothing allocated or uploaded, device
    // addresses stand-ins that are never read through (tinsel_hip_bake_source_desc: a scene description's baked header without a device)
    bool dry = false;
    template <class T> T* dry_address() const { return reinterpret_cast<T*>(uintptr_t(128)); }

    SceneBuild(tinsel_hip* r_, const tinsel_scene_desc* d, bool dry_ = false)
        : r(r_), sc(r_->scene), desc(d), tune(r_->tune), P(d->num_primitives), prims((size_t)P), mats((size_t)P), moving((size_t)P), dry(dry_)
    {
        for (int i = 0; i < P; ++i)
            if (desc->primitives[i].type == TINSEL_GEOM_MESH && mesh_bytes_estimate(desc->primitives[i].geo.mesh) > kSmallMeshBytes)
                sceneHasBigMesh = true;
    }

    // Where meshes live.  A scene all of whose meshes are small (<= 4 KB each; cornell's boxes) keeps them in the arena,
    // is staged whole into LDS and runs the fused kernel.  Once ONE mesh has to live in HBM the scene runs the split
    // pipeline, and there only meshes of a few triangles are worth walking inline from the arena: the others go to HBM
    // too and are walked by k_walk (glass.tin's 12-triangle cube: k_extend + k_shadow + k_walk 34.7 -> 31.3 ms; its
    // 2-triangle lamp stays inline -- every shadow ray enters its box).
    static size_t mesh_bytes_estimate(const tinsel_mesh_geometry& g)
    {
        return (size_t)g.num_nodes*32 + (size_t)(g.num_indices/3)*52 + (size_t)g.num_vertices*12;
    }
    bool lives_in_arena(size_t meshBytes, int numTris) const
    {
        // tinsel_hip_tuning::small_mesh_bytes: test / A-B knob (0 = every mesh lives in HBM, so the queue sort and k_walk see them all)
        if (tune.small_mesh_bytes >= 0)
            return meshBytes <= (size_t)tune.small_mesh_bytes;
        const int inlineMaxTris = tune.inline_max_tris >= 0 ? tune.inline_max_tris : kInlineMaxTris;
        return sceneHasBigMesh ? numTris <= inlineMaxTris && meshBytes <= kSmallMeshBytes : meshBytes <= kSmallMeshBytes;
    }

    // the steps, in the order tinsel_hip_create_tuned runs them
    int add_primitives();
    int add_mesh(const tinsel_mesh_geometry& g, Prim64& o);
    int scene_level();
    void mark_walked_and_quads();
    int assemble_arena();
    void set_scene_flags();
    int upload_probe();
    int stats_and_fit();
};

// device and LDS limits, the tuning
void create_limits(tinsel_hip* r, int device_index, const tinsel_hip_tuning* tuning)
{
    r->device = device_index;
    r->tune = tuning_from_caller(tuning);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_index) == hipSuccess)
    {
        r->numCUs = prop.multiProcessorCount;
        r->sharedMemLimit = (int)prop.sharedMemPerBlock;
    }
    // every kernel's dynamic-LDS limit is raised here, once, and the results are checked.  A runtime that refuses to raise one (it grants
    // less than the device reports) is not refused in turn: the renderer then plans every launch inside the 64 KB no attribute is needed
    // for -- 256-thread k_walk / k_swalk workgroups, no shading pools beside a large arena, k_seg_prefix's grids clamped -- and says so
    // once, by the kernel's name (a device that can render small scenes should)
    prepare_kernels_once(r);
    if (!r->prepRefused.empty() && r->sharedMemLimit > 65536)
    {
        fprintf(stderr, "tinsel_hip: the runtime refused %d B of dynamic LDS for %s: planning within 65536 B per workgroup\n", r->sharedMemLimit, r->prepRefused.c_str());
        r->sharedMemLimit = 65536;
        r->segPrefixLds = std::min(r->segPrefixLds, 65536 - 1024);
    }

    if (r->tune.batch_paths >= 65536)
    {
        r->maxBatchSlots = (size_t)r->tune.batch_paths;
        r->batchSlotsExplicit = true;
    }
}

// a mesh seen for the first time: validated, converted, its triangles gathered, into the arena or into HBM; its index into o.mesh
int SceneBuild::add_mesh(const tinsel_mesh_geometry& g, Prim64& o)
{
    const int numTris = g.num_indices/3;
    if (numTris <= 0 || !g.positions || !g.normals || !g.indices || !g.nodes || !g.cdf)
        return fail("create: mesh primitive with missing arrays");
    ConvertedBvh cb;
    // meshes that will live in HBM: the upper levels breadth-first (k_walk's LDS-resident top, tn_walk.h)
    if (!convert_bvh(g.nodes, g.num_nodes, numTris, lives_in_arena(mesh_bytes_estimate(g), numTris) ? 0 : kWalkTopNodes, cb))
        return fail("create: malformed mesh BVH");
    std::vector<Tri48> tris((size_t)numTris);
    for (int t = 0; t < numTris; ++t)
    {
        const int i0 = g.indices[t*3 + 0], i1 = g.indices[t*3 + 1], i2 = g.indices[t*3 + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= g.num_vertices || i1 >= g.num_vertices || i2 >= g.num_vertices)
            return fail("create: mesh index out of range");
        Tri48& T = tris[(size_t)t];
        T.ax = g.positions[i0].x; T.ay = g.positions[i0].y; T.az = g.positions[i0].z; T.i0 = i0;
        T.bx = g.positions[i1].x; T.by = g.positions[i1].y; T.bz = g.positions[i1].z; T.i1 = i1;
        T.cx = g.positions[i2].x; T.cy = g.positions[i2].y; T.cz = g.positions[i2].z; T.i2 = i2;
    }

    DevMesh dm;
    memset(&dm, 0, sizeof(dm));
    dm.root = cb.root;
    dm.numTris = numTris;
    dm.stackNeed = cb.maxLeafDepth + 1;
    dm.topCount = cb.topCount;
    dm.numInternal = (int32_t)cb.nodes.size();
    // one internal node over two one-triangle leaves (a quad): walked without stack or loop (ray_mesh_two_leaves)
    dm.twoLeaves = (cb.nodes.size() == 1 && !(cb.root & kLeafBit) && (cb.nodes[0].left & kLeafBit) && (cb.nodes[0].right & kLeafBit)) ? 1 : 0;
    const size_t meshBytes = cb.nodes.size()*sizeof(Node64) + tris.size()*sizeof(Tri48) + (size_t)g.num_vertices*12 + (size_t)numTris*4;
    if (lives_in_arena(meshBytes, numTris))
    {
        // offsets for now; turned into pointers once the arena has its device address
        dm.inArena = 1;
        dm.offNodes = (uint32_t)arena.add(cb.nodes.data(), cb.nodes.size());
        dm.offTris = (uint32_t)arena.add(tris.data(), tris.size());
        dm.offNormals = (uint32_t)arena.add(&g.normals[0].x, (size_t)g.num_vertices*3);
        dm.offCdf = (uint32_t)arena.add(g.cdf, (size_t)numTris);
    }
    else if (dry)
    {
        dm.nodes = dry_address<const Node64>(); dm.tris = dry_address<const Tri48>(); dm.normals = dry_address<const float>(); dm.cdf = dry_address<const float>();
    }
    else
    {
        dm.nodes = r->sceneMem.upload(cb.nodes.data(), cb.nodes.size());
        dm.tris = r->sceneMem.upload(tris.data(), tris.size());
        dm.normals = r->sceneMem.upload(&g.normals[0].x, (size_t)g.num_vertices*3);
        dm.cdf = r->sceneMem.upload(g.cdf, (size_t)numTris);
        if ((!cb.nodes.empty() && !dm.nodes) || !dm.tris || !dm.normals || !dm.cdf)
            return fail("create: device allocation failed (mesh)");
    }
    if (dm.stackNeed > maxMeshNeed)
        maxMeshNeed = dm.stackNeed;
    r->meshNumVertices.push_back(g.num_vertices);
    r->meshIndices.emplace_back(g.indices, g.indices + (size_t)numTris*3);
    r->meshRootLo.push_back(V3(g.nodes[0].lower.x, g.nodes[0].lower.y, g.nodes[0].lower.z));      // PrimitiveBounds reads nodes[0].bounds (intersection.h:928)
    r->meshRootHi.push_back(V3(g.nodes[0].upper.x, g.nodes[0].upper.y, g.nodes[0].upper.z));
    r->meshArea.push_back(g.area);
    o.mesh = (uint32_t)meshes.size();
    meshIndex[g.id] = o.mesh;
    meshes.push_back(dm);
    return 0;
}

// per primitive: material, pose, geometry
int SceneBuild::add_primitives()
{
    for (int i = 0; i < P; ++i)
    {
        const tinsel_primitive& p = desc->primitives[i];
        Prim64& o = prims[(size_t)i];
        memset(&o, 0, sizeof(o));

        make_material(p, mats[(size_t)i]);
        r->primEndScale.push_back(p.end_transform.s);
        if (p.light_samples > 0)
        {
            if (p.type == TINSEL_GEOM_PLANE)
                return fail("create: a plane cannot be a light (PrimitiveSample asserts, intersection.h:871-875)");
            lights.push_back(i);
            totalLightSamples += p.light_samples;
        }

        const bool isStatic = memcmp(&p.start_transform, &p.end_transform, sizeof(tinsel_transform)) == 0;
        const Xform xs = to_xform(p.start_transform), xe = to_xform(p.end_transform);
        r->primStart.push_back(xs);
        r->primEnd.push_back(xe);
        // InterpolateTransform(a, a, t) is t-independent: static primitives get it evaluated once, with the same function
        set_prim_pose(o, xs, xe, isStatic);
        // (a Moving64 slot for EVERY primitive, its own index: a static one may start to move, tinsel_hip_set_primitive_transform)
        o.moving = (uint32_t)i;
        moving[(size_t)i] = make_moving(xs, xe);

        if (p.type == TINSEL_GEOM_SPHERE)
        {
            o.type = kPrimSphere;
            o.g0 = p.geo.sphere.radius;
        }
        else if (p.type == TINSEL_GEOM_PLANE)
        {
            o.type = kPrimPlane;
            o.g0 = p.geo.plane.plane[0]; o.g1 = p.geo.plane.plane[1]; o.g2 = p.geo.plane.plane[2]; o.g3 = p.geo.plane.plane[3];
        }
        else if (p.type == TINSEL_GEOM_MESH)
        {
            o.type = kPrimMesh;
            const tinsel_mesh_geometry& g = p.geo.mesh;
            // Key on MeshGeometry::id and rewrite EVERY instance (the reference forgets both: render.cu:1000-1011)
            auto it = meshIndex.find(g.id);
            if (it != meshIndex.end())
                o.mesh = it->second;
            else if (add_mesh(g, o))
                return -1;
        }
        else
            return fail("create: unknown primitive type");
    }
    r->primMesh.assign((size_t)P, -1);
    r->lightPrims = lights;
    for (int i = 0; i < P; ++i)
    {
        set_prim_derived(prims[(size_t)i]);
        if (prims[(size_t)i].type == kPrimMesh)
            r->primMesh[(size_t)i] = (int)prims[(size_t)i].mesh;
    }
    return 0;
}

// the scene level (tn_host_scene.h; the plane table is decided in assemble_arena) and the traversal stack over it
int SceneBuild::scene_level()
{
    if (!build_scene_level(std::vector<tinsel_bvh_node>(desc->bvh_nodes, desc->bvh_nodes + desc->num_bvh_nodes), prims, {}, false, lvl))
        return fail("create: malformed scene BVH");
    const int need = lvl.bvh.maxLeafDepth + 1 + maxMeshNeed;
    r->stackNeed = pick_stack(need);
    if (r->stackNeed < 0)
        return fail("create: BVH too deep for the 156-entry LDS traversal stack");
    flatScan = lvl.everyPrimHasALeaf && P <= 64 && tune.flat_scan != 0;
    return 0;
}

// walked / binned primitives and quad records
void SceneBuild::mark_walked_and_quads()
{
    // primitives whose mesh lives in HBM (flat-scan scenes, the first 7): their leaf-box test sorts the ray queues
    // (k_generate, k_shade), and they are walked by k_walk ahead of the scan kernels (tn_walk.h).  That includes trees
    // that stay in L1/L2 (glass.tin's 1280-triangle sphere: 80 KB of nodes; its 12-triangle cube): what the lean kernel
    // buys there is ray replacement for incoherent bounces (glass, maxDepth 12: 924 -> 1001 Msamples/s with the sphere,
    // 1050 with the cube too; with k_walk's work list in image order the sphere had lost, 732 inline vs 657-690).
    const int walkMinTris = tune.walk_min_tris >= 0 ? tune.walk_min_tris : kInlineMaxTris + 1;
    r->binPrims.count = 0;
    r->walkPrims.count = 0;
    if (flatScan)
        for (int k = 0; k < P && r->binPrims.count < 7; ++k)
            if (prims[(size_t)k].type == kPrimMesh && !meshes[prims[(size_t)k].mesh].inArena)
            {
                r->binPrims.prim[r->binPrims.count++] = k;
                if (meshes[prims[(size_t)k].mesh].numTris >= walkMinTris)
                {
                    prims[(size_t)k].flags |= kPrimWalked | ((uint32_t)r->walkPrims.count << kPrimWalkLaneShift);
                    r->walkPrimMesh[r->walkPrims.count] = (int)prims[(size_t)k].mesh;
                    r->walkPrims.prim[r->walkPrims.count++] = k;
                }
            }
    // quads that ride in the arena: where their node, triangles and normals are goes into the primitive record, so that the scan reaches them
    // without the mesh table's record in between (one dependent fetch less per ray that enters the quad's box: every shadow ray of cornell)
    for (int k = 0; k < P; ++k)
        if (prims[(size_t)k].type == kPrimMesh && meshes[prims[(size_t)k].mesh].twoLeaves && meshes[prims[(size_t)k].mesh].inArena)
        {
            const DevMesh& qm = meshes[prims[(size_t)k].mesh];
            if (((qm.offNodes | qm.offTris | qm.offNormals | qm.offCdf) & 127u) != 0u || ((qm.offNodes | qm.offTris | qm.offNormals | qm.offCdf) >> 7) > 0xffffu)
                continue;
            Prim64& qp = prims[(size_t)k];
            qp.flags |= kPrimQuadArena;
            const uint32_t w0 = (qm.offNodes >> 7) | ((qm.offTris >> 7) << 16), w1 = (qm.offNormals >> 7) | ((qm.offCdf >> 7) << 16);
            memcpy(&qp.g0, &w0, 4); memcpy(&qp.g1, &w1, 4);
        }
    r->walkEnabled = tune.walk != 0;
#ifdef TN_WALK_PROF
    if (r->walkProf.alloc(16) == 0)
        (void)hipMemset(r->walkProf.get(), 0, 16*sizeof(unsigned long long));
#endif
}

// the plane table, the arena's assembly and upload, the DevScene pointers into it
int SceneBuild::assemble_arena()
{
    // one contiguous arena: scene BVH, Prim64, Mat128, moving poses, lights, mesh table (+ small meshes, added above)
    const size_t offNodes = arena.add(lvl.bvh.nodes.data(), lvl.bvh.nodes.size());
    const size_t offPrims = arena.add(prims.data(), prims.size());
    const size_t offMats = arena.add(mats.data(), mats.size());
    const size_t offMoving = arena.add(moving.data(), moving.size());
    std::vector<LightRec> lightRecs(lights.size());
    for (size_t l = 0; l < lights.size(); ++l)
        lightRecs[l] = { lights[l], mats[(size_t)lights[l]].lightSamples, mats[(size_t)lights[l]].rcpLightSamples, 0 };
    const size_t offLights = arena.add(lightRecs.data(), lightRecs.size());
    r->lightMats.clear();
    for (const int32_t l : lights)
        r->lightMats.push_back(mats[(size_t)l]);
    const size_t offMeshes = arena.add(meshes.data(), meshes.size());

    // The always-hit planes once more, four by four, for the flat scan (trace_flat): four IntersectRayPlane calls in a block are four
    // independent IEEE-division chains.  Where: scenes with a mesh in HBM (the split pipeline's kernels: glass k_extend -6 %, k_shadow
    // -5 %, round 4) and -- since k_bounce has the registers for it, round 5 -- fused scenes with at least one full block of four
    // (cornell 5283 -> 5450 Msamples/s, cfg1 +2.5 %); with fewer planes the table's remainder code only costs (gloss, env_loft -1 %:
    // profiles/r05_d_ab_plane_table_fused.md), so those keep the loop.
    int alwaysHitPlanes = 0;
    bool anyMeshInHbm = false;
    for (int k = 0; k < P; ++k)
    {
        alwaysHitPlanes += (prims[(size_t)k].type == kPrimPlane && lvl.boxes[(size_t)k].alwaysHit) ? 1 : 0;
        anyMeshInHbm = anyMeshInHbm || (prims[(size_t)k].type == kPrimMesh && !meshes[prims[(size_t)k].mesh].inArena);
    }
    if (flatScan && (alwaysHitPlanes >= 4 || anyMeshInHbm))
    {
        for (int k = 0; k < P; ++k)
            if (prims[(size_t)k].type == kPrimPlane && lvl.boxes[(size_t)k].alwaysHit)
                r->planeTablePrims.push_back(k);
        // Opposing planes of the table are tested as pairs (trace_flat), except where the fused kernel would defer mesh walks (two or more
        // mesh primitives, all in the arena): those instances of k_bounce have no scalar registers left for the pair block and carry none
        int meshPrimCount = 0;
        for (int k = 0; k < P; ++k)
            meshPrimCount += prims[(size_t)k].type == kPrimMesh ? 1 : 0;
        r->pairablePlanes = !(meshPrimCount >= 2 && !anyMeshInHbm);
        mark_plane_table(lvl, prims, r->planeTablePrims, pairs_planes(r, tune));
    }
    // (the table's slots are reserved once: pairs dissolve and form again as planes move, mark_plane_table keeps within them)
    const std::vector<float>& planeEq = lvl.planeEq;
    const std::vector<int32_t>& planeIdx = lvl.planeIdx;
    const size_t offBoxes = arena.add(lvl.boxes.data(), lvl.boxes.size());
    const size_t offPlaneEq = arena.add(planeEq.data(), planeEq.size());
    const size_t offPlaneIdx = arena.add(planeIdx.data(), planeIdx.size());
    arena.bytes.resize((arena.bytes.size() + 127) & ~size_t(127), 0);

    unsigned char* arenaDev = dry ? dry_address<unsigned char>() : r->sceneMem.upload(arena.bytes.data(), arena.bytes.size());
    if (!arenaDev)
        return fail("create: device allocation failed (scene arena)");
    // small meshes: offsets -> device pointers, in the host image of the mesh table, then upload once more
    DevMesh* hm = reinterpret_cast<DevMesh*>(&arena.bytes[offMeshes]);
    for (size_t m = 0; m < meshes.size(); ++m)
    {
        if (hm[m].inArena)
        {
            hm[m].nodes = reinterpret_cast<const Node64*>(arenaDev + hm[m].offNodes);
            hm[m].tris = reinterpret_cast<const Tri48*>(arenaDev + hm[m].offTris);
            hm[m].normals = reinterpret_cast<const float*>(arenaDev + hm[m].offNormals);
            hm[m].cdf = reinterpret_cast<const float*>(arenaDev + hm[m].offCdf);
        }
    }
    if (!dry && !meshes.empty() && hipMemcpy(arenaDev + offMeshes, hm, sizeof(DevMesh)*meshes.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail("create: device allocation failed (scene arena)");
    r->meshesRef.assign(hm, hm + meshes.size());
    r->meshesNow = r->meshesRef;

    sc.arena = arenaDev;
    sc.arenaBytes = (uint32_t)arena.bytes.size();
    const size_t ldsLimit = tune.arena_lds_limit >= 0 ? (size_t)tune.arena_lds_limit : kArenaLdsLimit;
    sc.arenaLdsBytes = (arena.bytes.size() <= ldsLimit && tune.lds_scene != 0) ? sc.arenaBytes : 0u;
    sc.nodes = reinterpret_cast<const Node64*>(arenaDev + offNodes);
    sc.prims = reinterpret_cast<const Prim64*>(arenaDev + offPrims);
    sc.mats = reinterpret_cast<const Mat128*>(arenaDev + offMats);
    sc.moving = reinterpret_cast<const Moving64*>(arenaDev + offMoving);
    sc.lights = reinterpret_cast<const LightRec*>(arenaDev + offLights);
    sc.meshes = reinterpret_cast<const DevMesh*>(arenaDev + offMeshes);
    sc.numMeshes = (int)meshes.size();
    sc.primBoxes = reinterpret_cast<const PrimBox*>(arenaDev + offBoxes);
    sc.planeEq = reinterpret_cast<const float4*>(arenaDev + offPlaneEq);
    sc.planeIdx = reinterpret_cast<const int32_t*>(arenaDev + offPlaneIdx);
    adopt_scene_level(r, lvl);
    r->arenaOffNodes = offNodes;
    r->arenaOffBoxes = offBoxes;
    r->arenaOffPrims = offPrims;
    r->arenaOffMoving = offMoving;
    r->arenaOffMats = offMats;
    r->primsHost = prims;
    return 0;
}

// the scene flags: hasMedia, flatScan, deferMeshes, sortQueues, sceneEnclosed, allInArena; counts and sky
void SceneBuild::set_scene_flags()
{
    sc.hasMedia = 0;
    for (const Mat128& mm : mats)
        if (mm.absorption[0] != 0.0f || mm.absorption[1] != 0.0f || mm.absorption[2] != 0.0f)
            sc.hasMedia = 1;
    r->anyTransmission = std::any_of(mats.begin(), mats.end(), [](const Mat128& mm) { return mm.transmission != 0.0f; });
    r->anySubsurface = std::any_of(mats.begin(), mats.end(), [](const Mat128& mm) { return !is_plus_zero(mm.subsurface); });
    sc.flatScan = flatScan ? 1 : 0;
    {
        int meshPrimCount = 0;
        for (int k = 0; k < P; ++k)
            meshPrimCount += prims[(size_t)k].type == kPrimMesh ? 1 : 0;
        sc.deferMeshes = (meshPrimCount >= 2) ? 1 : 0;
    }
    // Fused kernel: sort the next bounce's queue by "meets the box of a bounded primitive" (tn_isect.h) when the
    // scene is open.  Measured (cornell-sized frames, fused kernel): env_loft (1 plane) +16 %, gloss (1 plane) +4 %;
    // the closed boxes cornell / cornell+probe (5 planes, every NEE ray aimed at the light mesh) -4 %: the test and
    // the second append cost more than the plane-only waves save.
    {
        int planes = 0;
        for (int k = 0; k < P; ++k)
            planes += lvl.boxes[(size_t)k].alwaysHit ? 1 : 0;
        sc.sortQueues = (sc.flatScan && planes <= 2 && planes < P) ? 1 : 0;
    }
    // two infinite planes with opposite normals (a floor and a ceiling): every ray between them that is not parallel to
    // them hits one -- a scene no ray leaves, whatever else is in it (cornell.tin, glass.tin)
    for (int i = 0; i < P && !r->sceneEnclosed; ++i)
        for (int j = i + 1; j < P && !r->sceneEnclosed; ++j)
            if (prims[(size_t)i].type == kPrimPlane && prims[(size_t)j].type == kPrimPlane)
            {
                const Prim64 &a = prims[(size_t)i], &b = prims[(size_t)j];
                const float d = a.g0*b.g0 + a.g1*b.g1 + a.g2*b.g2;
                const float la = sqrtf(a.g0*a.g0 + a.g1*a.g1 + a.g2*a.g2), lb = sqrtf(b.g0*b.g0 + b.g1*b.g1 + b.g2*b.g2);
                r->sceneEnclosed = la > 0.0f && lb > 0.0f && d < -0.99f*la*lb;
            }
    bool all = sc.arenaLdsBytes != 0;
    for (const DevMesh& dmesh : meshes)
        all = all && dmesh.inArena;
    sc.allInArena = all ? 1 : 0;
    sc.numPrims = P;
    sc.numLights = (int)lights.size();
    sc.horizon[0] = desc->sky_horizon.x; sc.horizon[1] = desc->sky_horizon.y; sc.horizon[2] = desc->sky_horizon.z;
    sc.zenith[0] = desc->sky_zenith.x; sc.zenith[1] = desc->sky_zenith.y; sc.zenith[2] = desc->sky_zenith.z;
}

int SceneBuild::upload_probe()
{
    const size_t n = (size_t)desc->probe_width*desc->probe_height;
    if (!desc->probe_data || !desc->probe_pdf_x || !desc->probe_cdf_x || !desc->probe_pdf_y || !desc->probe_cdf_y || n == 0)
        return fail("create: probe marked valid but arrays missing");
    if (dry)
    {
        sc.probe.valid = 1;
        return 0;
    }
    sc.probe.data = (const float4*)r->sceneMem.upload((const float*)desc->probe_data, n*4);
    sc.probe.pdfX = r->sceneMem.upload(desc->probe_pdf_x, n);
    sc.probe.cdfX = r->sceneMem.upload(desc->probe_cdf_x, n);
    sc.probe.pdfY = r->sceneMem.upload(desc->probe_pdf_y, (size_t)desc->probe_height);
    sc.probe.cdfY = r->sceneMem.upload(desc->probe_cdf_y, (size_t)desc->probe_height);
    sc.probe.width = desc->probe_width;
    sc.probe.height = desc->probe_height;
    sc.probe.valid = 1;
    if (!sc.probe.data || !sc.probe.pdfX || !sc.probe.cdfX || !sc.probe.pdfY || !sc.probe.cdfY)
        return fail("create: device allocation failed (probe)");
    return 0;
}

// statistics; then the traversal stacks (+ the staged arena) must fit a workgroup's LDS: give the arena up first, then refuse
int SceneBuild::stats_and_fit()
{
    r->neePerPath = totalLightSamples + (r->scene.probe.valid ? 1 : 0);
    r->scene.totalLightSamples = r->neePerPath;
    if (!dry && (r->statsDev.alloc((size_t)kStatShards*kStatWords) ||
        hipMemset(r->statsDev.get(), 0, sizeof(unsigned long long)*kStatShards*kStatWords) != hipSuccess))
        return fail("create: device allocation failed (stats)");
    if (stack_bytes(r) > (size_t)r->sharedMemLimit && r->scene.arenaLdsBytes)
    {
        r->scene.arenaLdsBytes = 0;
        r->scene.allInArena = 0;
    }
    if (stack_bytes(r) > (size_t)r->sharedMemLimit)
        return fail("create: the traversal stacks of this scene need " + std::to_string(stack_bytes(r)) + " B of LDS per workgroup, the device offers " + std::to_string(r->sharedMemLimit));
    return 0;
}

// create's steps on `r` (limits and tuning set); dry: SceneBuild::dry
int build_scene(tinsel_hip* r, const tinsel_scene_desc* desc, bool dry)
{
    memset(&r->scene, 0, sizeof(r->scene));
    SceneBuild b(r, desc, dry);
    if (b.add_primitives() || b.scene_level())
        return -1;
    b.mark_walked_and_quads();
    if (b.assemble_arena())
        return -1;
    b.set_scene_flags();
    if ((desc->probe_valid && b.upload_probe()) || b.stats_and_fit())
        return -1;
    return 0;
}

// the workgroup LDS limit a scene description is planned with where no device is asked: gfx950's
constexpr int kDescSharedMemLimit = 160*1024;

// tinsel_hip_bake_source's body (tn_host_api.h has the live entry, this file the description's)
long long bake_source_of(const tinsel_hip* r, char* out_text, unsigned long long capacity, char* out_key65, int* out_bakeable)
{
    const std::string text = bake_text(bake_tables(r));
    if (out_text && capacity > 0)
    {
        const size_t n = std::min<size_t>(text.size(), (size_t)capacity - 1);
        memcpy(out_text, text.data(), n);
        out_text[n] = 0;
    }
    if (out_key65)
        memcpy(out_key65, sha256_hex(text).c_str(), 65);
    if (out_bakeable)
    {
        std::string why;
        *out_bakeable = plans_fit_closed(r, &why) ? 1 : 0;
        if (!*out_bakeable)
            g_error = "bake_source: not bakeable: " + why;
    }
    return (long long)text.size();
}

} // namespace

extern "C" {


const char* tinsel_hip_last_error(void) { return g_error.c_str(); }

void tinsel_hip_tuning_init(tinsel_hip_tuning* t)
{
    if (t)
        *t = tuning_defaults();
}

tinsel_hip* tinsel_hip_create(const tinsel_scene_desc* desc, int device_index) { return tinsel_hip_create_tuned(desc, device_index, nullptr); }

tinsel_hip* tinsel_hip_create_tuned(const tinsel_scene_desc* desc, int device_index, const tinsel_hip_tuning* tuning)
{
    if (!desc || !desc->primitives || desc->num_primitives <= 0 || !desc->bvh_nodes || desc->num_bvh_nodes <= 0)
    {
        fail("create: empty scene (Scene::Build must have run)");
        return nullptr;
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    {
        fail("create: no HIP device visible -- this library has no CPU fallback");
        return nullptr;
    }
    if (device_index < 0 || device_index >= ndev)
    {
        fail("create: bad device index");
        return nullptr;
    }
    HIP_TRY_NULL(hipSetDevice(device_index));

    std::unique_ptr<tinsel_hip> r(new tinsel_hip());
    create_limits(r.get(), device_index, tuning);
    if (build_scene(r.get(), desc, false))
        return nullptr;
    return r.release();
}

long long tinsel_hip_bake_source_desc(const tinsel_scene_desc* desc, const tinsel_hip_tuning* tuning, char* out_text, unsigned long long capacity,
                                      char* out_key65, int* out_bakeable)
{
    if (!desc || !desc->primitives || desc->num_primitives <= 0 || !desc->bvh_nodes || desc->num_bvh_nodes <= 0)
        return fail("bake_source_desc: empty scene (Scene::Build must have run)");
    // create's host half on a renderer that owns nothing on any device: the same records, offsets and plan inputs
    std::unique_ptr<tinsel_hip> r(new tinsel_hip());
    r->tune = tuning_from_caller(tuning);
    r->sharedMemLimit = kDescSharedMemLimit;
    if (build_scene(r.get(), desc, true))
        return -1;
    return bake_source_of(r.get(), out_text, capacity, out_key65, out_bakeable);
}

void tinsel_hip_destroy(tinsel_hip* r)
{
    if (!r)
        return;
    (void)hipSetDevice(r->device);
    lookahead_release(r);
    (void)hipDeviceSynchronize();
    comm_release(r);
    if (r->walkProf)
    {
        unsigned long long wp[16] = { 0 };
        (void)hipMemcpy(wp, r->walkProf.get(), sizeof(wp), hipMemcpyDeviceToHost);
        const double tot = (double)(wp[0] + wp[1] + wp[2] + wp[3] + wp[4]);
        fprintf(stderr, "k_walk profile: cycles refill %.1f%% node %.1f%% tri %.1f%% pop %.1f%% loop %.1f%% | iterations %llu refills %llu node-phases %llu tri-phases %llu | "
                "lanes/node-phase %.1f lanes/tri-phase %.1f lanes/refill %.1f | waves %llu cycles/wave %.0f cycles/iteration %.0f cycles/refill %.0f cycles/node-phase %.0f cycles/tri-phase %.0f\n",
                100.0*wp[0]/tot, 100.0*wp[1]/tot, 100.0*wp[2]/tot, 100.0*wp[3]/tot, 100.0*wp[4]/tot, wp[5], wp[6], wp[7], wp[8],
                (double)wp[9]/std::max(1ull, wp[7]), (double)wp[10]/std::max(1ull, wp[8]), (double)wp[11]/std::max(1ull, wp[6]),
                wp[12], (double)wp[13]/std::max(1ull, wp[12]), tot/std::max(1ull, wp[5]), (double)wp[0]/std::max(1ull, wp[6]),
                (double)wp[1]/std::max(1ull, wp[7]), (double)wp[2]/std::max(1ull, wp[8]));
    }
    delete r;       // every buffer, stream and event goes with its owner (tn_host_own.h)
}

} // extern "C"
