// trace_lean_scene.inc — part (B) of the lean tracer (trace_lean.hpp::traceLean, which includes it twice; every unit): the scene-graph walk of the lanes that stand
// between two meshes, to the point where each of them has entered a mesh, finished its ray or (kNodesChunked, kNodesTlas)
// stands before its next candidate window. One text for all forms: each form's way to the next node it has to look at
// comes first, under `if constexpr`, then the node visit all forms share.
//
// A textual include because traceLean needs it at two places — inside the "mask, walk again" loop of the windowed forms and
// without that loop for the others — and neither a loop that runs once for the other forms nor a local lambda leaves their
// code alone (profiles/lean_fold_resources.txt). The order of the statements is the order the four separate tracers had them
// in, and `rest` is declared where each of them declared it — after the kNodesWalk test, before the windows' `continue` —:
// declared ahead of the kNodesWalk test it changes that form's register allocation.
    // ---------------------------------------------------------------- (B) scene-graph walk
    while (has && !inMesh && !(kWindows && needMask)) {       // (lanes leave this loop one by one)
      WF_PHASE(tally, 3);                                     // walk steps
      // the form's loop head: on to the next node the ray can reach, or out of the loop
      if constexpr (!kMask) {
        if (nodeI >= sc.nNodes) {                             // testNode of the root has returned
          done = true;                                        // (committed at the next refill)
          has = false;
          break;
        }
      }
      if constexpr (NODES == kNodesWalk) {
        // No candidate mask: every lane walks the node list on its own, as the reference's recursion does: the node's padded world
        // box first (the test a mask bit stands for; conservative: a ray that misses it within [0, hit.t] fails the exact test
        // below, for this node and for every node of its subtree), a miss jumps over the subtree through the node's skip link, a
        // hit goes on to the exact test in the node's space. A ray costs the nodes it visits, not the nodes the scene has.
        if (!rayIsWorld) { const LeanRay r = fetch(slot); ray = makeRay(r.o + 0.0f, r.d + 0.0f); rayIsWorld = true; }
        const f4 wlo = sc.nodeWorld[2u * nodeI], whi = sc.nodeWorld[2u * nodeI + 1u];
        const float wmin[3] = {wlo.x, wlo.y, wlo.z}, wmax[3] = {whi.x, whi.y, whi.z};
        float dw;
        WF_PHASE(tally, 4);                                   // padded-box tests
        YART_COUNT(nBox, 1);
        if (!testBox(ray, 0.0f, hit.t + (fabsf(hit.t) * 1e-4f + 1e-3f), wmin, wmax, dw)) { nodeI = __builtin_bit_cast(uint32_t, wlo.w); continue; }   // (the skip link rides in the box record)
      }
      if constexpr (kWindows) {
        if (nodeI >= candBase + 64u) {                        // beyond this window: the next one first (kNodesTlas: the next non-empty one)
          if constexpr (NODES == kNodesChunked) candBase = nodeI & ~63u;
          needMask = true;
          if constexpr (NODES == kNodesChunked) { if (skipUntil < nodeI) skipUntil = nodeI; }
          break;
        }
      }
      // the candidates from nodeI on (kNodesWalk keeps no mask: the node it stands at is one)
      const unsigned long long rest = kMask ? (nodeI < 64u ? (cand >> nodeI) : 0ull) : kWindows ? cand >> (nodeI - candBase) : 1ull;
      if constexpr (kWindows) {
        if (rest == 0ull) { nodeI = candBase + 64u; continue; }
      }
      if (kMask && rest == 0ull) {                            // kNodesMask: testNode of the root has returned
        done = true;                                          // (committed at the next refill)
        has = false;
      } else {
        if constexpr (NODES != kNodesWalk) nodeI += uint32_t(__builtin_ctzll(rest));
        // the node visit: exact node box in the node's space, then the mesh's root box
        const NodeDev& nd = sc.nodes[nodeI];
        if (!((MODE & TRAV_IDENTITY) || (nd.pad[0] & 1u))) {
          // transformed node (its padded world box is known to be hit): the exact object-space ray
          const LeanRay r = fetch(slot);                      // the exact world ray (ray.o/d carry +0.0f)
          f3 oo, od;
          objectRay(sc, nodeI, r.o, r.d, oo, od);
          ray = makeRay(oo, od); rayIsWorld = false;
        } else if (!rayIsWorld) {
          const LeanRay r = fetch(slot); ray = makeRay(r.o + 0.0f, r.d + 0.0f); rayIsWorld = true;
        }
        float dd;
        YART_COUNT(nBox, 1);
        if (!testBox(ray, tMin, hit.t, nd.bmin, nd.bmax, dd) || hit.t < dd) nodeI = nd.skip;   // (mask bits of the subtree may remain set: skipped by index)
        else {
          bool entered = false;
          if (nd.mesh >= 0) {
            const MeshDev& mesh = sc.meshes[nd.mesh];
            if (!(NEE && kFast && didHit && !mesh.hasAlpha)) {  // pruning of occluded shadow rays (traverse.hpp)
              nodes = sc.bvhNodes + mesh.nodeOffset;
              leaves = sc.leafTris + mesh.leafOffset;
              meshHasAlpha = mesh.hasAlpha != 0;
              const BvhNode root = nodes[0];
              YART_COUNT(nBox, 1);
              if (testBox(ray, tMin, hit.t, root.bmin, root.bmax, d)) {       // testBVH entry
                inMesh = true; entered = true;
                leftFirst = root.leftFirst; span = root.span; stackIdx = 0; meshDidHit = false;
              }
            }
          }
          if (!entered) nodeI++;
        }
      }
    }
