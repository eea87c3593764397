/*
 * ecm_mesh.h -- the mesh entries of libecm_hip.so: an indexed, welded, oriented triangle mesh of the zero level of a TSDF volume
 * (ecm_volume.h), extracted on the device by marching tetrahedra.
 *
 * A seventh header beside ecm_hip.h, ecm_geometry.h, ecm_rectify.h, ecm_temporal.h, ecm_motion.h and ecm_volume.h, with its own
 * prefix (ecms_).  The conventions are ecm_hip.h's: plain pointers and ints, every pointer a DEVICE pointer the caller owns,
 * `stream` a hipStream_t passed as void* (NULL = default stream), work enqueued asynchronously, 0 on success, a negative ECM_E*
 * code of ecm_hip.h on a bad argument (ecm_error_string names it) or the positive hipError_t of a failed launch.
 *
 * Every operation below is one IEEE fp64 operation in the stated order, without fused multiply-adds, unless it says fp32; an fp32
 * operand of an fp64 operation is widened first, and (float) rounds once to nearest.  row(M, r, a, b, c) is ecm_volume.h's:
 * ((M[r][0] * a + M[r][1] * b) + M[r][2] * c) + M[r][3].
 *
 * Volume and points.  tsdf, wsum [nz,ny,nx] fp32 as in ecm_volume.h, every dim >= 2; grid point (i, j, k) -- i along x -- has the
 *   linear index (k * ny + j) * nx + i.  A point is USABLE iff wsum > min_weight (compared in fp32; a NaN wsum fails) and tsdf is
 *   finite.  A usable point is POSITIVE iff tsdf > 0, and negative otherwise: +0.0 and -0.0 are negative, as in the raycast's
 *   f0 > 0 >= f1.
 * Cubes and tetrahedra.  Cube (i, j, k), 0 <= i <= nx-2 and likewise along y and z, is LIVE iff its eight corners are usable.
 *   Every cube is split into the six Kuhn (Freudenthal) tetrahedra: tetrahedron p = 0..5 is the p-th permutation (a0, a1, a2) of
 *   the axes (0, 1, 2) in lexicographic order, with the corners c0 = (0,0,0), c1 = c0 + e_a0, c2 = c1 + e_a1, c3 = (1,1,1) of the
 *   cube.  The split is the same in every cube, so neighbouring cubes agree on the diagonal of the face they share.  The CASE of
 *   a tetrahedron has bit c set iff corner c is positive.
 * Edges and vertices.  Every edge of a tetrahedron runs from a grid point p in one of seven directions: dir 0..6 = (1,0,0),
 *   (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1).  Its SLOT is (p, dir).  A slot carries a vertex iff its two ends differ
 *   in sign and at least one live cube contains the edge (up to four cubes for an axis edge, two for a face diagonal, one for the
 *   body diagonal): so every vertex is referenced by a face and every slot a face references has a vertex.  Vertices are numbered
 *   in the order (linear index of p, then dir).
 * Vertex position.  With t0 = tsdf at p and t1 = tsdf at p + dir:  a = t0 / (t0 - t1);  g[axis] = p[axis] + dir[axis] * a;
 *   vertices[n][r] = (float) row(M, r, g[0], g[1], g[2]), r = 0..2.  M is an fp64 4x4 row-major grid-to-output matrix whose
 *   bottom row is (0, 0, 0, 1) and is not read: there is no division.
 * Normals (normals may be NULL).  The gradient G(p) of tsdf at a grid point, per axis with unit vector e:  t(p+e) - t(p-e) where
 *   both neighbours are in the grid and usable; else t(p+e) - t(p) where that neighbour is; else t(p) - t(p-e) where that one is;
 *   else 0.  With G0 = G(p), G1 = G(p + dir):  n[axis] = G0[axis] + a * (G1[axis] - G0[axis]);
 *   m[r] = (M[r][0] * n[0] + M[r][1] * n[1]) + M[r][2] * n[2];  len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
 *   normals[n][r] = (float)(m[r] / len), or +0.0 three times where len is 0 or not finite.  It points to the positive side (free
 *   space) provided that M's linear part is a positive multiple of a rotation, which is the caller's to supply.
 * Vertex weight (weight may be NULL).  weight[n] = (float)(w0 + a * (w1 - w0)) of the two wsum, widened.
 * Triangles.  The live cubes in linear order, in each the tetrahedra 0..5, in each the triangles of its case in table order.  The
 *   table, with XY the vertex on the edge between the corners X and Y of the tetrahedron:
 *     a lone corner L (exactly one corner positive, or exactly one negative), the others A < B < C:  one triangle (LA, LB, LC);
 *     two and two, the positive corners P < P', the negative ones N < N':  the quad (PN, PN', P'N', P'N) = (q0, q1, q2, q3) as
 *       the triangles (q0, q1, q2) and (q0, q2, q3);
 *     orientation: with every vertex at the midpoint of its edge, a triangle (v0, v1, v2) for which
 *       ((v1 - v0) x (v2 - v0)) . (centroid of the positive corners - centroid of the negative corners) < 0 has its last two
 *       entries swapped (the product is never 0 for a Kuhn tetrahedron): seen from the positive side every triangle is
 *       counter-clockwise.
 *   faces[f] holds the three int32 vertex numbers of triangle f.
 * Properties.  Away from the boundary of the grid and from cubes that are not live the surface is a closed, consistently oriented
 *   2-manifold: every directed edge is used once and its reverse once.  A tsdf of +-0 puts a at 0 or 1, so several vertices then
 *   coincide: the zero-area triangles this gives are KEPT, and nothing is welded by position (vertices are shared by slot only).
 */
#ifndef ECM_MESH_H
#define ECM_MESH_H

#include "ecm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The points of one tile of the stream compaction (2048), and the points of a classification brick along axis 0, 1, 2 = x, y, z
 * (16, 4, 4; 0 for any other axis).  No GPU needed. */
int ecms_mesh_tile(void);
int ecms_mesh_brick(int axis);

/* The bytes of scratch both entries below need for a volume of nx * ny * nz points: a state word and a vertex base index per
 * point and two counts per tile, 8 * points + 8 * ceil(points / ecms_mesh_tile()) rounded up to 16.  0 where the entries refuse
 * the sizes (a dim < 2, more than 2^27 points).  No GPU needed. */
long long ecms_mesh_scratch_bytes(int nx, int ny, int nz);

/* Count the vertices and triangles of the mesh: counts[0] and counts[1], int64, written on the device.  Four launches: bricks of
 * 16 x 4 x 4 points with a halo of one point on every side classify their points from usable and sign bits staged in LDS (the
 * live flag of the point's cube, the 7-bit mask of its slots, the triangles of its cube, the signs of the cube's corners: one
 * state word per point in scratch); the counts of each linear tile; one workgroup scans the tile counts.  No atomics, no
 * workgroup waits for another: bit-reproducible.  scratch (any 4-byte alignment) must then go unchanged to ecms_mesh_emit_fwd.
 * ECM_EINVAL, before any device work: a null tsdf, wsum, counts or scratch; nx, ny or nz < 2; min_weight not finite or < 0;
 * counts or scratch equal to one another or to tsdf or wsum; scratch_bytes below ecms_mesh_scratch_bytes(nx, ny, nz).
 * ECM_EUNSUP, before any launch: nx * ny * nz > 2^27 (at or below it 7 * points and 12 * cubes stay below 2^31, which int32 faces
 * need), or more tiles than the one-workgroup scan takes (2^24 - 1; not reachable within 2^27 points). */
int ecms_mesh_count_fwd(const float* tsdf, const float* wsum, long long* counts, void* scratch, long long scratch_bytes, int nx,
                        int ny, int nz, float min_weight, void* stream);

/* Write the mesh that ecms_mesh_count_fwd counted, from the scratch it left, for the same tsdf, wsum, sizes and min_weight:
 * vertices [n_vertices,3] fp32, faces [n_faces,3] int32 and, where given, normals [n_vertices,3] fp32 and weight [n_vertices]
 * fp32.  Two launches: the vertices (which also leave every point's first vertex number in scratch), then the faces, which find
 * the number of a slot through that number plus the set bits of the point's mask below dir.  n_vertices and n_faces are the
 * CAPACITIES of the outputs in rows: every store is bounded by them, a capacity below the count is legal (the rows that fit are
 * written, the rest dropped), and rows beyond the count are not written.  Every read of scratch lies within
 * ecms_mesh_scratch_bytes(nx, ny, nz); a scratch that is not the count pass's gives wrong rows, never a store out of bounds.
 * ECM_EINVAL, before any device work: a null tsdf, wsum, M, vertices, faces or scratch; nx, ny or nz < 2; min_weight not finite
 * or < 0; n_vertices or n_faces < 0; vertices, faces, normals, weight or scratch equal to one another or to tsdf, wsum or M;
 * scratch_bytes below ecms_mesh_scratch_bytes(nx, ny, nz).  ECM_EUNSUP, before any launch: as ecms_mesh_count_fwd. */
int ecms_mesh_emit_fwd(const float* tsdf, const float* wsum, const double* M, float* vertices, int* faces, float* normals,
                       float* weight, void* scratch, long long scratch_bytes, long long n_vertices, long long n_faces, int nx, int ny,
                       int nz, float min_weight, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECM_MESH_H */
