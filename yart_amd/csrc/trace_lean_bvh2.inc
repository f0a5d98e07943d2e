// trace_lean_bvh2.inc — part (C) of the lean tracer (trace_lean.hpp::traceLean, its only include site; every unit): the while-while BVH
// traversal, step for step and test for test the reference's (cpu/ray-integrator.cpp:84-160: near child first,
// far child pushed with its entry distance, pop-cull d < hit.t, leaf triangles in index order), written for the
// scalar unit: the step is straight-line, the lane state the loop changes is integers in VGPRs (cur = link word,
// d, sp, live), every decision is a v_cndmask, and only the two stack accesses are predicated regions. (A first
// form kept that state as C++ bools, which the compiler holds as wave masks and merges with an s_andn2 / s_and /
// s_or triple at every divergent join: one SALU per VALU instruction, profiles/r1_pmc_sq_summary.txt. Variants
// measured and dropped — masked loads, a postponed leaf, in-kernel alpha peek, any-order shadow walk, packed fp32
// slab products — are recorded in profiles/r2_lean_kernel_variants.txt and DESIGN §7; the code is in git history.)
    // ------------------------------------------------------------------ (C) BVH traversal, while-while
    {
      uint32_t cur = packLink(leftFirst, span);                 // index | alpha bit | span << 27 (31 = 31 or more: leafSpan)
      uint32_t live = inMesh ? 1u : 0u;
      const uint32_t wasLive = live;
      // NEE pruning of the lean shadow kernels (traverse.hpp): an occluded ray only enters subtrees with alpha-tested
      // triangles. (didHit || meshDidHit) changes in the leaf phase only.
#define LEAN2_VISIT(link, dist) ((dist) < hit.t && (!(NEE && kFast) || !occl || ((link) & kLinkAlphaBit)))
      for (;;) {
        const bool occl = didHit || meshDidHit;
        // inner nodes and pops until every live lane stands at a leaf it must test
        for (;;) {
          const bool visit = LEAN2_VISIT(cur, d);
          const bool isLeaf = (cur >> kSpanShift) != 0u;
          if (!(live != 0u && !(isLeaf && visit))) break;       // (lanes leave the loop one by one)
          WF_PHASE(tally, 0);                                   // inner / pop steps
          // lanes that only pop read the root's children (always valid, L1 resident): no branch around the loads
          const BvhNode* pair = nodes + (visit ? (cur & kLinkIndexMask) : 1u);
          const BvhNode c1 = pair[0], c2 = pair[1];
          if (visit) YART_COUNT(nBox, 2);
          if (visit) WF_PHASE(tally, 7);                        // (of the inner / pop steps: lanes that test a pair of boxes)
          float d1, d2;
          bool hit1, hit2;
          testBox2(ray, tMin, hit.t, c1, c2, hit1, hit2, d1, d2);
          hit1 = hit1 && visit; hit2 = hit2 && visit;
          const bool firstNear = hit1 && !(hit2 && d1 > d2);
          const uint32_t l1 = c1.leftFirst, l2 = c2.leftFirst;      // (the device's link word carries the saturated span: host_scene.hpp)
          const uint32_t nearLink = firstNear ? l1 : l2, farLink = firstNear ? l2 : l1;
          const float nearD = firstNear ? d1 : d2, farD = firstNear ? d2 : d1;
          if (hit1 && hit2) stackPush(stk, stackIdx++, farLink, farD);
          const bool any = hit1 || hit2;
          uint32_t popLink = cur; float popD = d;
          const bool canPop = !any && stackIdx != 0u;
          if (canPop) stackPop(stk, --stackIdx, popLink, popD);
          cur = any ? nearLink : popLink;
          d = any ? nearD : popD;
          live = (any || canPop) ? live : 0u;                   // stack empty: testBVH returns
          // the stragglers of the inner phase do not hold up the lanes waiting at their leaves:
          // they step again after the leaf phase, together with the lanes that come back from it
          if (uint32_t(__popcll(__ballot(true))) < kLeanInnerMin) break;
        }
        // leaves: triangles in index order
        if (live != 0u && (cur >> kSpanShift) != 0u && LEAN2_VISIT(cur, d)) {
          WF_PHASE(tally, 2);                                   // leaf visits
          const uint32_t first = cur & kLinkIndexMask;
          const uint32_t nLeaf = leafSpan(leaves, first, cur >> kSpanShift);
          for (uint32_t i = 0; i < nLeaf; i++) {
            WF_PHASE(tally, 1);                                 // triangle tests
            const LeafTri tr = leaves[first + i];
            YART_COUNT(nTri, 1);
            const f3 p0 = mk3(tr.p0[0], tr.p0[1], tr.p0[2]);
            const f3 edge1 = mk3(tr.e1[0], tr.e1[1], tr.e1[2]);
            const f3 edge2 = mk3(tr.e2[0], tr.e2[1], tr.e2[2]);
            bool accepted = false;
            do {
              const f3 rayEdge2 = cross(ray.d, edge2);
              const float det = dot(edge1, rayEdge2);
              if (double(fabsf(det)) < 1e-12) break;
              const float invDet = 1.0f / det;
              const f3 b = ray.o - p0;
              const float u = dot(b, rayEdge2) * invDet;
              if (u < 0.0f || u > 1.0f) break;
              const f3 bEdge1 = cross(b, edge1);
              const float v = dot(ray.d, bEdge1) * invDet;
              if (v < 0.0f || u + v > 1.0f) break;
              const float t = dot(edge2, bEdge1) * invDet;
              if (t <= tMin || hit.t <= t) break;
              if (kFast) {
                if (tr.matFlags & ((NEE && !(didHit || meshDidHit)) ? (MAT_HAS_ALPHA | MAT_TRANSPARENT) : MAT_HAS_ALPHA)) {
                  pendingRetry = true;                          // the general kernel traces this ray again
                  break;
                }
                // an occluded shadow ray accepts nothing further: its interval stays what it was at the first hit, and every
                // triangle of the leaves it still visits is looked at (traverse.hpp::traverseMesh, the leaf loop's end)
                if (NEE && (didHit || meshDidHit)) break;
              } else if (tr.matFlags & (MAT_HAS_ALPHA | MAT_TRANSPARENT)) {
                // alpha cut-outs and NEE-transparent surfaces (ray-integrator.cpp:198-221)
                f2 uv; f3 n;
                interpUVN(sc, tr.triIdx, u, v, uv, n);
                const MaterialDev& mt = sc.materials[tr.material];
                if (tr.matFlags & MAT_HAS_ALPHA) {
                  const float alpha = matAlpha(sc, mt, uv);
                  if (alpha < 1.0f && get1D(smp, scfg) > alpha) break;
                }
                if (NEE && (tr.matFlags & MAT_TRANSPARENT)) {
                  attenuation *= absDot(n, ray.d) * matBase(sc, mt, uv);
                  break;
                }
              }
              hit.t = t; hit.u = u; hit.v = v; hit.tri = tr.triIdx; hit.node = nodeI;
              hit.backSide = (det < 0 ? 1u : 0u) | (tr.material << 1);
              accepted = true;
            } while (false);
            if (pendingRetry) break;
            meshDidHit |= accepted;
            if (NEE && (kFast ? accepted : meshDidHit)) break;
          }
          // (an occluded lean shadow ray has nothing left to find in a mesh without alpha-tested triangles)
          if (pendingRetry) live = 0u;
          else if (stackIdx == 0u || (NEE && kFast && meshDidHit && !meshHasAlpha)) live = 0u;
          else stackPop(stk, --stackIdx, cur, d);
        }
        if (uint32_t(__popcll(__ballot(live != 0u))) < 64u - kRefill + 1u) break;
      }
#undef LEAN2_VISIT
      // lanes that left their BVH in this round (testBVH returned, or the ray goes to the general kernel)
      if (wasLive != 0u && live == 0u) {
        inMesh = false;
        if (pendingRetry) has = false;
        else { didHit |= meshDidHit; nodeI++; }
      }
      leftFirst = cur & ((1u << kSpanShift) - 1u); span = cur >> kSpanShift;
    }
