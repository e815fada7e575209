// Arithmetic of the coordinate-map builders (lerf_coords.hip), HIP-free on the host side: one source for the kernels and for the
// host twins (lerf_coords_*_host), so a machine without a GPU tests the same statements.  Float64, only + - * /, comparisons,
// selects and bit-casts, FMA contraction off, NO LIBRARY FUNCTION on either side: the square root and the arc tangents the lens
// models need are sqrt_pm, atan_pm and atan2_pm below, written in these operations (a few ulp from libm's, NOT equal to them), so
// the device and the host agree BIT FOR BIT, like project_point against coords.from_homography(arithmetic="device").  Every
// function returns the UNCLIPPED (row, col) of one output pixel (i, j) of the whole map; the remap clips (remap_pixel).
//
// The exact operation order (tests/coords_ref.py restates it; every product and sum is rounded, sums run left to right):
//
//   HOMOGRAPHY  p = inverse matrix m[9]:  project_unclipped (lerf_host_geometry.h)
//                 X = m0*x + m1*y + m2,  Y = m3*x + m4*y + m5,  Wh = m6*x + m7*y + m8,  x = (double)j, y = (double)i
//                 col = X / Wh,  row = Y / Wh
//   RADIAL      p = cr, cc, no, ni, hr, hc, k1, k2  (coords.radial's scalars: centre, the two half-diagonals, the half-extents
//               (oH - 1) / 2 and (oW - 1) / 2 of the WHOLE output):
//                 ur = (i - hr) / no,  uc = (j - hc) / no,  r2 = ur*ur + uc*uc
//                 f = (1 + k1*r2) + (k2*r2)*r2
//                 row = cr + (ur*f)*ni,  col = cc + (uc*f)*ni
//   BROWN       p = m[9] (inv(new_K . R), the host's), fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6
//               (cv::initUndistortRectifyMap's pinhole + Brown-Conrady model, no skew):
//                 (y, x) = project_unclipped(m, i, j)              -- u = j, v = i through the matrix, the two divisions
//                 r2  = x*x + y*y
//                 rad = (1 + r2*(k1 + r2*(k2 + r2*k3))) / (1 + r2*(k4 + r2*(k5 + r2*k6)))
//                 xy  = x*y
//                 xd  = (x*rad + (2*p1)*xy) + p2*(r2 + 2*(x*x))
//                 yd  = (y*rad + p1*(r2 + 2*(y*y))) + (2*p2)*xy
//                 col = fx*xd + cx,  row = fy*yd + cy
//   sqrt_pm(x)  a bit-cast start and six Heron passes (within 1 ulp of the exact root; 0 -> +0, x < 0 or NaN -> NaN, +inf -> +inf):
//                 xs = x * 2^108 if x < 2^-1022 (a subnormal: exact), else x
//                 y = the double whose bits are (bits(xs) >> 1) + 0x1FF8000000000000          (within 6.1 % of the root)
//                 six times:  y = 0.5 * (y + xs / y)
//                 y * 2^-54 if x < 2^-1022 (exact); then the selects of 0, +inf, NaN
//   atan_pm(x)  fdlibm's reduction onto four anchors and its odd polynomial (within 1 ulp; NaN -> NaN, +-inf -> +-pi/2 rounded to
//               a double, |x| < 2^-29 -> x), ax = |x| by a select:
//                 ax < 7/16:   t = ax / 1                              hi = lo = 0
//                 ax < 11/16:  t = (2*ax - 1) / (2 + ax)               hi + lo = atan(1/2)
//                 ax < 19/16:  t = (ax - 1) / (ax + 1)                 hi + lo = atan(1)
//                 ax < 39/16:  t = (ax - 1.5) / (1 + 1.5*ax)           hi + lo = atan(3/2)
//                 else:        t = -1 / ax                             hi + lo = atan(inf) = pi/2
//               (numerator, denominator, hi, lo by selects, ONE division)
//                 z = t*t,  w = z*z
//                 s1 = z*(a0 + w*(a2 + w*(a4 + w*(a6 + w*(a8 + w*a10))))),  s2 = w*(a1 + w*(a3 + w*(a5 + w*(a7 + w*a9))))
//                 r = hi - ((t*(s1 + s2) - lo) - t);  -r if x < 0: atan_pm(-x) = -atan_pm(x) bit for bit
//   atan2_pm(y, x)  a = atan_pm(y / x), then by selects (pi = pi_hi + pi_lo, two doubles):
//                 x > 0:  a
//                 x < 0:  (a + pi_lo) + pi_hi if y >= 0 -- y = +0 and y = -0 both count as + -- else (a - pi_lo) - pi_hi
//                 x == 0: +pi/2 if y > 0, -pi/2 if y < 0, 0 if y == 0
//                 a NaN in y or x: NaN.  (inf, inf) is NaN, unlike libm's; atan2_pm(-y, x) = -atan2_pm(y, x) bit for bit, y != 0
//   FISHEYE     p = m[9] (inv(new_K . R), the host's), fx, fy, cx, cy, k1, k2, k3, k4   (cv::fisheye::initUndistortRectifyMap's
//               equidistant model, no skew):
//                 (y, x) = project_unclipped(m, i, j),  Wh = m6*u + m7*v + m8  (project_unclipped's statement)
//                 not Wh > 0 (a ray behind the camera, Wh = 0, a NaN):  (NaN, NaN), by a select
//                 r = sqrt_pm(x*x + y*y),  th = atan_pm(r),  th2 = th*th
//                 thd = th*(1 + th2*(k1 + th2*(k2 + th2*(k3 + th2*k4))))
//                 s = thd / r,  1 where r == 0 (a select)
//                 col = fx*(x*s) + cx,  row = fy*(y*s) + cy
//   EQUIRECT    p = m[9] (inv(K_view . R)), sx, sy, cxp, cyp   (a pinhole view of an equirectangular panorama; for a panorama
//               [Hp][Wp] with pixel centres sx = Wp / (2 pi), sy = Hp / pi, cxp = (Wp - 1) / 2, cyp = (Hp - 1) / 2):
//                 u = (double)j, v = (double)i
//                 dx = m0*u + m1*v + m2,  dy = m3*u + m4*v + m5,  dz = m6*u + m7*v + m8          (no division)
//                 lon = atan2_pm(dx, dz),  h = sqrt_pm(dx*dx + dz*dz),  lat = atan2_pm(dy, h)
//                 col = cxp + sx*lon,  row = cyp + sy*lat          (the seam lon = +-pi is clipped like any border)
//   mesh        ctrl [gh][gw][2], vertices align-corners over the WHOLE output [full_h][full_w]; per axis (rows: n = full_h,
//               g = gh, k = i):
//                 u = ((double)k * (double)(g - 1)) / (double)(n - 1)           (0 when n == 1)
//                 bilinear: a0 = min((int)floor(u), g - 2), t = u - a0, taps a0, a0 + 1, weights 1 - t, t
//                 bicubic:  f = (int)floor(u), t = u - f, taps f - 1 .. f + 2 clamped to [0, g - 1], Keys weights with A = -0.75 in
//                           torch's upsample_bicubic2d forms:  c1(x) = ((A + 2)*x - (A + 3))*x*x + 1,
//                           c2(x) = ((A*x - 5*A)*x + 8*A)*x - 4*A,  w = c2(t + 1), c1(t), c1(1 - t), c2(2 - t)
//               value = sum_a wr[a] * (sum_b wc[b] * ctrl[a][b]), both sums left to right starting from their first product
//   compose     C[i][j] = A(B[i][j]), A [aH][aW][2] sampled bilinearly at the position B holds; per axis (rows: n = aH, v = row):
//                 r = clip of v onto [0, n - 1] (clip_coord: -inf -> 0, +inf -> n - 1)
//                 i0 = min((int)floor(r), n - 2)  (0 when n == 1),  t = r - i0,  weights 1 - t, t
//               value = acc over rows a = 0, 1 of wr[a] * (acc over columns b = 0, 1 of wc[b] * A[i0 + a][j0 + b]), every acc
//               starting at +0.0 and adding its terms in order; a term whose weight is exactly 0 is NOT added and its entry of
//               A is NOT read.  A NaN in either coordinate of B[i][j]: (NaN, NaN), nothing of A is read.  No value of B forms
//               an address outside A: the position is clipped before any conversion to int, and a tap outside A (n == 1,
//               or r on the last row) has weight exactly 0.
//   invert      G[q] = the u with F(u) = q, F [fH][fW][2] (fH, fW >= 2) read as its bilinear interpolant under compose's per-axis rule
//               (compose_axis: clip onto [0, n - 1], i0 = min(floor(r), n - 2), t = r - i0, weights w0 = 1 - t, w1 = t), by Newton's
//               method on the piecewise-bilinear patch; q = ((double)(i0 + i), (double)(j0 + j)).
//               start, when no init map gives it (invert_start; it does not depend on the tile):
//                 A = F[0][0],  P = F[fH - 1][0],  Q = F[0][fW - 1]
//                 B = (P - A) / (double)(fH - 1),  C = (Q - A) / (double)(fW - 1)          (per component)
//                 det = B.r*C.c - B.c*C.r,  d = q - A
//                 u.r = (d.r*C.c - C.r*d.c) / det,  u.c = (B.r*d.c - B.c*d.r) / det
//                 det == 0 or not finite (det - det != 0):  u = ((double)(fH - 1) / 2, (double)(fW - 1) / 2)
//               iteration k = 0 .. max_iter - 1 (invert_point):
//                 a NaN in u: (NaN, NaN), nothing is read
//                 R = compose_axis(u.r, fH), Cx = compose_axis(u.c, fW)
//                 P00 = F[R.i0][Cx.i0], P01 = F[R.i0][Cx.i0 + 1], P10 = F[R.i0 + 1][Cx.i0], P11 = F[R.i0 + 1][Cx.i0 + 1]: ALL FOUR
//                 are read, whatever their weights (a NaN corner of the cell makes the entry NaN)
//                 V = R.w0*(Cx.w0*P00 + Cx.w1*P01) + R.w1*(Cx.w0*P10 + Cx.w1*P11)   (per component; compose_point's value of a
//                                                                                     finite cell, up to the sign of a zero)
//                 e = V - q;  a NaN in e: (NaN, NaN);  |e.r| <= tol and |e.c| <= tol: the result is the clipped u, (r, c), where
//                 r = clip_coord(u.r, fH - 1), c = clip_coord(u.c, fW - 1)
//                 Jr = Cx.w0*(P10 - P00) + Cx.w1*(P11 - P01),  Jc = R.w0*(P01 - P00) + R.w1*(P11 - P10)   (dV/dr, dV/dc)
//                 det = Jr.r*Jc.c - Jr.c*Jc.r;  det == 0 or not finite: (NaN, NaN)
//                 u.r = r - (e.r*Jc.c - Jc.r*e.c) / det,  u.c = c - (Jr.r*e.c - Jr.c*e.r) / det
//               no iteration met tol: (NaN, NaN) -- a target F does not reach.  No value of F, init or q forms an address
//               outside F: u goes through compose_axis (clipped in floating point before the conversion to int, fH, fW >= 2).
//   invert_raster   G[q] = the u with T(u) = q, T the PIECEWISE-LINEAR interpolant of F [fH][fW][2] (fH, fW >= 2) over two triangles a
//               cell (not invert's bilinear patch), by rasterising every triangle into the tile and keeping, per pixel, the smallest
//               64-bit key; q = ((double)(i0 + i), (double)(j0 + j)).  Cell (i, j), 0 <= i < fH - 1, 0 <= j < fW - 1, P00 = F[i][j],
//               P01 = F[i][j + 1], P10 = F[i + 1][j], P11 = F[i + 1][j + 1]:
//                 triangle t = 2*(i*(fW - 1) + j)   (even):  A = P00, B = P01, C = P10
//                 triangle t + 1                    (odd):   A = P11, B = P10, C = P01
//               edge(P, Q, q) = (Q.c - P.c)*(q.r - P.r) - (Q.r - P.r)*(q.c - P.c)      ((Q - P) x (q - P); the identity's triangles are > 0)
//               set-up of one triangle (raster_setup); a triangle that fails a test is SKIPPED: it contributes nothing, forms no address:
//                 the six coordinates finite (v - v == 0); with depth, no NaN among zA, zB, zC
//                 area2 = edge(A, B, C);  area2 != 0 and finite;  not (orient > 0 and area2 < 0), not (orient < 0 and area2 > 0)
//                 per axis (rows: v = A.r, B.r, C.r):  lo = ceil(min v), hi = floor(max v)   (min / max by selects, left to right)
//                 (hi - lo) + 1 > (double)max_span on either axis: skipped   (the tear rule, BEFORE the clip; in float64)
//                 lo = max(lo, (double)first), hi = min(hi, (double)last), first / last the tile's first and last row (column);
//                 lo > hi on either axis: skipped;  only now the conversion to int
//               per pixel q of the box, rows outer, columns inner (tri_edges: each edge with its endpoints in ascending index i*fW + j,
//               negated where the triangle A -> B -> C -> A runs the other way, so the two triangles on an edge see ONE number):
//                 even:  e_c = edge(A, B, q),   e_a = edge(B, C, q),   e_b = -edge(A, C, q)
//                 odd:   e_c = -edge(B, A, q),  e_a = -edge(C, B, q),  e_b = edge(C, A, q)
//                 inside (closed):  area2 > 0: e_a >= 0, e_b >= 0, e_c >= 0;  area2 < 0: all three <= 0
//                 l_b = e_b / area2,  l_c = e_c / area2                                                  (tri_value)
//                 even:  u = ((double)i + l_c, (double)j + l_b);   odd:  u = ((double)(i + 1) - l_c, (double)(j + 1) - l_b)
//                 z = (float)(zA + (l_b*(zB - zA) + l_c*(zC - zA)))   in float64 from the float32 depths, rounded once; a NaN z is the
//                 canonical quiet NaN 0x7FC00000;  without depth z = +0.0f and l_b, l_c are not needed                (tri_depth)
//                 key = (sortable(z) << 32) | t,  sortable(b) = ~b if b has its sign bit, else b | 0x80000000, b the bits of z
//                 keys[q] = min(keys[q], key)     (the device: one 64-bit atomic min; an integer min does not depend on the order)
//               resolve, per entry: keys[q] all ones (untouched): (NaN, NaN);  else t = the low 32 bits, cell = t >> 1, i = cell / (fW - 1),
//               j = cell % (fW - 1), the triangle's three vertices are read again, area2 = edge(A, B, C), tri_edges, tri_value: u.
//   trimesh     out[q] = the attribute an INDEXED triangle mesh holds at pixel q = ((double)(i0 + i), (double)(j0 + j)): pos [V][2] the vertices in
//               the output frame, attr [Va][2] what the map holds at a vertex, faces [F][3] indices into pos, attr_faces [F][3] into attr (null:
//               faces), depth [V] float32 and w [V] float32 / float64 optional (promoted exactly).  invert_raster's edge, inside test, tri_depth
//               and key, over faces of any size; face f has vertices A, B, C = pos at faces[f][0..2] (indices ia, ib, ic).
//               set-up of one face (TriMesh::read, tri_setup); a face that fails a test is SKIPPED: it contributes nothing, forms no address:
//                 (uint32)index < (uint32)V for the three of faces, < (uint32)Va for the three of attr_faces (of faces when null): ONE unsigned
//                 compare each, BEFORE any vertex is read, so -1, V and 2^31 - 1 read nothing               (tri_index_ok)
//                 the six coordinates finite (v - v == 0); with depth, no NaN among zA, zB, zC
//                 with w: wA, wB, wC finite and > 0   (no near-plane clipping: a face that crosses w = 0 is skipped)
//                 area2 = edge(A, B, C);  area2 != 0 and finite (a repeated index gives exactly 0);  not (orient > 0 and area2 < 0), not
//                 (orient < 0 and area2 > 0)
//                 per axis:  lo = ceil(min v), hi = floor(max v);  max_span > 0 and (hi - lo) + 1 > (double)max_span: skipped  (tri_axis:
//                 raster_axis with the tear rule optional);  the clip onto the tile in floating point, lo > hi: skipped, only then the int
//               per pixel q of the clipped box (tri_pixel; tri_edges_indexed: every directed edge of A -> B -> C -> A from its LOWER vertex
//               index, so two faces that share an edge by index compare ONE number against 0 with opposite signs):
//                 e_c = ia < ib ? edge(A, B, q) : -edge(B, A, q)
//                 e_a = ib < ic ? edge(B, C, q) : -edge(C, B, q)
//                 e_b = ic < ia ? edge(C, A, q) : -edge(A, C, q)            (on grid_faces' triangulation: tri_edges' numbers, even and odd)
//                 inside (closed): tri_inside;  z = tri_depth(e, area2, zA, zB, zC), +0.0f without depth;  key = raster_key(z, f)
//                 keys[q] = min(keys[q], key)
//               resolve, per entry (TriResolveOp, tri_attr): keys[q] all ones: (NaN, NaN) and NaN in depth_out;  else f = the low 32 bits, the
//               indices, positions, attributes aA, aB, aC (and w) are read again, area2 = edge(A, B, C), tri_edges_indexed, then per component
//                 l_b = e_b / area2,  l_c = e_c / area2
//                 without w:  u = aA + (l_b*(aB - aA) + l_c*(aC - aA))
//                 with w:     ia = 1 / wA, ib = 1 / wB, ic = 1 / wC
//                             d = ia + (l_b*(ib - ia) + l_c*(ic - ia))
//                             n = aA*ia + (l_b*(aB*ib - aA*ia) + l_c*(aC*ic - aA*ia)),  u = n / d
//                 depth_out = the float whose bits invert sortable() on the key's high word (key_depth): b = s & 0x7FFFFFFF if s has its top bit,
//                 else ~s;  u is rounded once to out's dtype
//               The device bins the faces into item tiles of kTileRows x kTileCols = 4 x 16 pixels aligned to the tile's own rows and columns
//               (tri_tiles: tr0 = (r0 - i0) / 4 .. (r1 - i0) / 4, tc0 = (c0 - j0) / 16 .. (c1 - j0) / 16) and draws one (face, tile) item a wave;
//               the host loops over faces and boxes.  An integer min does not depend on the order: neither the tiles nor the chunks show.
//   trimesh backward (tri_attr_bwd, tri_face_terms; lerf_coords_trimesh_bwd)   the adjoint of the resolve at FIXED VISIBILITY: pixel q
//               belongs to the face f in the low word of keys[q]; coverage and the depth test get no gradient.  g = grad_out[q].
//               per face, once (tri_grads):  area2 = edge(A, B, C);  the constant gradients of the barycentrics, (d/dq.r, d/dq.c):
//                 Ga = ((C.c - B.c) / area2, -((C.r - B.r) / area2)),  Gb = ((A.c - C.c) / area2, -((A.r - C.r) / area2)),
//                 Gc = ((B.c - A.c) / area2, -((B.r - A.r) / area2))
//               per pixel:  l_b = e_b / area2,  l_c = e_c / area2 (tri_attr's),  l_a = (1 - l_b) - l_c
//                 without w:  attr_k = (l_k*g.r, l_k*g.c)                                            -- 6 sums S_k a face
//                 with w:     ia, ib, ic, d, n, u = n / d as in tri_attr;  m_k = (l_k*i_k) / d
//                             h_k = ((a_k.r - u.r)*g.r + (a_k.c - u.c)*g.c) * i_k
//                             v.r = ((h_a*Ga.r + h_b*Gb.r) + h_c*Gc.r) / d,  v.c likewise with the .c of Ga, Gb, Gc
//                             attr_k = (m_k*g.r, m_k*g.c),  pos_k = (-(l_k*v.r), -(l_k*v.c)),  w_k = -(m_k*h_k)       -- 15 sums a face
//               THE ORDER OF THE SUMS IS PART OF THE CONTRACT (tri_bwd_thread): one face = 4 x 64 slots (kTriBwdWaves); slot (r, l) owns lane
//               pixel l (row l / 16, column l % 16) of the item tiles k = r, r + 4, ... < ntr*ntc of the face's clipped box (tri_tiles: tile
//               k is row k / ntc, column k % ntc) and adds its pixels' terms in ascending k into sums that start at +0.0; a pixel adds only
//               when it lies in the box, its key is not all ones and the key's low word is f.  Then per sum the butterfly over the 64
//               lanes x[l] = x[l] + x[l ^ m], m = 32, 16, 8, 4, 2, 1, and the four slots r as ((p0 + p1) + p2) + p3.
//               the face's terms (tri_face_terms):  with w the sums themselves;  without w  attr_k = S_k,  w_k = 0 and
//                 Jrr = (aA.r*Ga.r + aB.r*Gb.r) + aC.r*Gc.r,  Jrc = the same with Ga.c, Gb.c, Gc.c,  Jcr, Jcc = the same from the a.c
//                 pos_k = (-(Jrr*S_k.r + Jcr*S_k.c), -(Jrc*S_k.r + Jcc*S_k.c));  a NaN term is the canonical quiet NaN
//               the vertices: element v of grad_pos (grad_w; grad_attr through attr_faces) = what it held + the terms of the corners that name
//               v, one after the other in ascending (face, corner) order.  A face the forward's set-up skips adds nothing anywhere.
//   compose backward (compose_bwd_point; aH, aW >= 2)   one entry with inner point (row, col) and upstream g = (g.r, g.c):
//                 a NaN in row or col: nothing is read, nothing is scattered, the inner gradient is (0, 0) whatever g holds (a select)
//                 R = compose_axis(row, aH), Cx = compose_axis(col, aW), wr = {R.w0, R.w1}, wc = {Cx.w0, Cx.w1}: the forward's
//               outer gradient (scatter_taps), taps in the order (0,0) (0,1) (1,0) (1,1); a tap with wr[a] == 0 or wc[b] == 0 is skipped
//               and forms no address:
//                 w = wr[a]*wc[b];  grad_A[R.i0 + a][Cx.i0 + b] += (w*g.r, w*g.c)
//               inner gradient: P00, P01, P10, P11 as in invert_point, ALL FOUR read whatever their weights (cell_jacobian):
//                 Jr = Cx.w0*(P10 - P00) + Cx.w1*(P11 - P01),  Jc = R.w0*(P01 - P00) + R.w1*(P11 - P10)      (invert_point's statements)
//                 d.r = Jr.r*g.r + Jr.c*g.c  if 0 <= row <= aH - 1, else 0;  d.c = Jc.r*g.r + Jc.c*g.c  if 0 <= col <= aW - 1, else 0
//               (torch.clamp's backward: the border passes, outside and +-inf are blocked by a select, so a NaN sum behind a blocked
//               clip is 0; a NaN that passes is returned as the canonical quiet NaN, so the host and the device agree on its bits).  The derivative of the plain bilinear formula with i0 held constant: at an integer position it is that of
//               cell i0 = min(floor(r), n - 2), and a NaN corner makes the inner gradient NaN even where the forward did not read it.
//   invert backward (invert_bwd_point; fH, fW >= 2)   one entry G = (r, c) of the inverse with upstream g; F(G[q]) = q gives
//               dG = -J^-1 dF(G), so the gradient on F is the bilinear scatter of v = -J^-T g:
//                 a NaN in r or c: nothing is read or scattered
//                 R = compose_axis(r, fH), Cx = compose_axis(c, fW);  P00 .. P11 all read;  a NaN in any of their 8 values: nothing
//                 Jr, Jc as above;  det = Jr.r*Jc.c - Jr.c*Jc.r;  det == 0 or not finite: nothing
//                 v.r = -(Jc.c*g.r - Jr.c*g.c) / det,  v.c = -(Jr.r*g.c - Jc.r*g.r) / det
//                 scatter_taps of v into grad_F at the cell (R.i0, Cx.i0), the same rule and order as the outer gradient
//               init, max_iter and tol have no gradient.  Neither backward forms an address outside its map: the cell comes from
//               compose_axis and n >= 2 puts i0 + 1 <= n - 1.
//   model backward (model_point_bwd<MODEL>; every model)   one entry (i, j) with upstream g = (g.r, g.c): the hand-written
//               reverse mode of model_point, dp[k] = d(row)/d(p[k]) * g.r + d(col)/d(p[k]) * g.c for EVERY entry of the parameter
//               vector (radial's geometry scalars no, ni, hr, hc included; the caller keeps what it fits).  The forward is
//               recomputed by the forward's own statements; (row, col) = model_point(p, i, j).
//                 row or col not finite (row - row != 0: Wh == 0, fisheye's Wh <= 0, an overflow, a NaN parameter): dp[k] = 0 for every k, whatever g
//                 holds -- a select, as in compose_bwd_point; this is NOT autograd's rule (autograd returns NaN or inf there).  A
//                 NaN in g at a finite point propagates.
//               HOMOGRAPHY  x = (double)j, y = (double)i, X, Y, Wh, col, row as above
//                 dX = g.c / Wh,  dY = g.r / Wh,  dWh = -((g.c*col + g.r*row) / Wh)
//                 dp[0..2] = dX*x, dX*y, dX;  dp[3..5] = dY*x, dY*y, dY;  dp[6..8] = dWh*x, dWh*y, dWh
//               RADIAL      ur, uc, r2, f as above
//                 dp[cr] = g.r,  dp[cc] = g.c
//                 dp[ni] = g.r*(ur*f) + g.c*(uc*f)
//                 ar = g.r*ni,  ac = g.c*ni                                  -- d/d(ur*f), d/d(uc*f)
//                 df = ar*ur + ac*uc
//                 dp[k1] = df*r2,  dp[k2] = df*(r2*r2)
//                 dr2 = df*(k1 + (2*k2)*r2)
//                 dur = ar*f + dr2*(2*ur),  duc = ac*f + dr2*(2*uc)
//                 dp[hr] = -(dur / no),  dp[hc] = -(duc / no),  dp[no] = -((dur*ur + duc*uc) / no)
//               BROWN       u = (double)j, v = (double)i, X, Y, Wh, x = X / Wh, y = Y / Wh, r2, xy as above, and
//                 num = 1 + r2*(k1 + r2*(k2 + r2*k3)),  den = 1 + r2*(k4 + r2*(k5 + r2*k6)),  rad = num / den
//                 a1 = r2 + 2*(x*x),  a2 = r2 + 2*(y*y),  xd, yd as above
//                 dp[fx] = g.c*xd,  dp[cx] = g.c,  dp[fy] = g.r*yd,  dp[cy] = g.r
//                 dxd = g.c*fx,  dyd = g.r*fy
//                 dp[p1] = dxd*(2*xy) + dyd*a2,  dp[p2] = dxd*a1 + dyd*(2*xy)
//                 drad = dxd*x + dyd*y,  dnum = drad / den,  dden = -((drad*rad) / den)
//                 r4 = r2*r2,  r6 = r4*r2
//                 dp[k1] = dnum*r2, dp[k2] = dnum*r4, dp[k3] = dnum*r6, dp[k4] = dden*r2, dp[k5] = dden*r4, dp[k6] = dden*r6
//                 dr2 = (dnum*(k1 + r2*(2*k2 + r2*(3*k3))) + dden*(k4 + r2*(2*k5 + r2*(3*k6)))) + (dxd*p2 + dyd*p1)
//                 dx = (((dxd*rad + dxd*((2*p1)*y)) + (dxd*p2)*(4*x)) + dyd*((2*p2)*y)) + dr2*(2*x)
//                 dy = (((dyd*rad + (dyd*p1)*(4*y)) + dxd*((2*p1)*x)) + dyd*((2*p2)*x)) + dr2*(2*y)
//                 dX = dx / Wh,  dY = dy / Wh,  dWh = -((dx*x + dy*y) / Wh)
//                 dp[0..2] = dX*u, dX*v, dX;  dp[3..5] = dY*u, dY*v, dY;  dp[6..8] = dWh*u, dWh*v, dWh
//               FISHEYE     u, v, Wh, x, y, r, th, th2, thd, s as above, xs = x*s, ys = y*s
//                 dp[fx] = g.c*xs,  dp[cx] = g.c,  dp[fy] = g.r*ys,  dp[cy] = g.r
//                 dxs = g.c*fx,  dys = g.r*fy,  ds = dxs*x + dys*y
//                 dthd = ds / r,  drs = -((ds*s) / r);  both 0 where r == 0 (a select)               -- s = thd / r
//                 th3 = th*th2, th5 = th3*th2, th7 = th5*th2, th9 = th7*th2
//                 dp[k1] = dthd*th3, dp[k2] = dthd*th5, dp[k3] = dthd*th7, dp[k4] = dthd*th9
//                 dth = dthd*(1 + th2*(3*k1 + th2*(5*k2 + th2*(7*k3 + th2*(9*k4)))))
//                 dr = drs + dth / (1 + r*r)                                                           -- d atan(r) = dr / (1 + r*r)
//                 dv = dr / (2*r);  0 where r == 0 (a select)                                        -- d sqrt(v) = dv / (2 sqrt(v))
//                 dx = dxs*s + dv*(2*x),  dy = dys*s + dv*(2*y)
//                 dX = dx / Wh,  dY = dy / Wh,  dWh = -((dx*x + dy*y) / Wh);  dp[0..8] as for BROWN
//               at the principal ray (r == 0) the model is the pinhole's, col = fx*x + cx: what is left is its gradient
//               EQUIRECT    u, v, dx, dy, dz, lon, h, lat as above
//                 dp[cxp] = g.c,  dp[sx] = g.c*lon,  dp[cyp] = g.r,  dp[sy] = g.r*lat
//                 dlon = g.c*sx,  dlat = g.r*sy
//                 n2 = dy*dy + h*h                                           -- d atan2(a, b) = (b*da - a*db) / (a*a + b*b)
//                 ddy = (h*dlat) / n2,  dh = -((dy*dlat) / n2);  both 0 where n2 == 0 (a select)
//                 v2 = dx*dx + dz*dz,  dv = dh / (2*h)
//                 ddx = (dz*dlon) / v2 + dv*(2*dx),  ddz = -((dx*dlon) / v2) + dv*(2*dz);  dv, ddx, ddz 0 where h == 0 (a select:
//                 at a pole lon is the constant 0 and lat the constant +-pi/2)
//                 dp[0..2] = ddx*u, ddx*v, ddx;  dp[3..5] = ddy*u, ddy*v, ddy;  dp[6..8] = ddz*u, ddz*v, ddz
//   build backward (lerf_coords_build_bwd / _host)   grad_params[s][k] += sum over the entries of map s of dp[k].  THE ORDER OF THE SUM IS
//               PART OF THE CONTRACT: a function of (oH, oW, n_sets) only, the same on the device and in the host twin, so two runs and
//               the two sides agree bit for bit.  With C = 64 columns and R = 64 rows per band (kBwdCols, kBwdBand), nbx = ceil(oW / C),
//               nby = ceil(oH / R), nblk = nbx*nby:
//                 pass 1, band (bx, by) of set s, its 4 x 64 "lanes" (w, l), w = 0 .. 3, l = 0 .. 63, column j = bx*C + l:
//                   acc = +0.0;  for t = 0 .. 15: i = by*R + w + 4*t;  if i < oH and j < oW: acc = acc + dp[k] of entry (i, j)
//                   (a lane or row outside the map adds nothing, which equals adding +0.0: acc is never -0.0)
//                 the 64 lanes of w by the tree  for off = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l + off]  (l < off), result v[0]
//                 partial[s][k][by*nbx + bx] = ((v0[w = 0] + v0[1]) + v0[2]) + v0[3]
//                 pass 2, per (s, k): 64 lanes, lane l: acc = +0.0; for b = l, l + 64, ... < nblk: acc = acc + partial[s][k][b];
//                   the same tree;  grad_params[s][k] = grad_params[s][k] + v[0]   (one writer: a plain load-add-store)
//               The workspace holds the partials: n_sets * n_params * nblk doubles (2160 x 3840, brown: 60 * 34 * 21 * 8 B = 343 KB a set).
//   reproject   (reproject_point<KIND>)   p = m[9] (K_dst . R . inv(K_src), row-major), q[3] (K_dst . t); one entry (i, j) of view A with
//               depth `depth` (a float32 depth is promoted exactly) lands at (row, col) of view B with depth zo there:
//                 x = (double)j,  y = (double)i                            -- (i, j) of the WHOLE map: the caller adds the tile's origin
//                 a0 = (m0*x + m1*y) + m2,  a1 = (m3*x + m4*y) + m5,  a2 = (m6*x + m7*y) + m8
//                 LERF_DEPTH_Z       (z = depth):  X = a0*z + q0,  Y = a1*z + q1,  W = a2*z + q2,  zo = W
//                 LERF_DEPTH_INVERSE (d = depth):  X = a0 + q0*d,  Y = a1 + q1*d,  W = a2 + q2*d,  zo = W / d,  +inf where d == 0 (a select)
//                 col = X / W,  row = Y / W
//                 valid:  Z: z > 0, z - z == 0, W > 0;   INVERSE: d >= 0, d - d == 0, W > 0   (false for a NaN anywhere)
//                 not valid: row = col = zo = NaN, by selects (fisheye's rule for a ray behind the camera)
//               the map entry is stored like every map's (float32: rounded once), zo as float32 (rounded once; beyond float32: +inf)
//   reproject backward (reproject_point_bwd<KIND>)   one entry with upstream g = (g.r, g.c) on (row, col) and gz on zo (0 when there is no
//               upstream for zo); the forward is recomputed by the statements above.
//                 not valid, or row or col not finite: dp[k] = 0 for every k and d depth = 0, whatever g and gz hold (selects)
//                 dX = g.c / W,  dY = g.r / W,  dWm = -((g.c*col + g.r*row) / W)
//                 Z:        gze = gz if zo is finite (zo - zo == 0), else 0;   dW = dWm + gze
//                           d depth = (dX*a0 + dY*a1) + dW*a2
//                           A = (dX*z, dY*z, dW*z),  Q = (dX, dY, dW)
//                 INVERSE:  gzd = gz / d and gzz = gzd*zo if zo is finite, else both 0 (a point at infinity takes nothing from gz);  dW = dWm + gzd
//                           d depth = ((dX*q0 + dY*q1) + dW*q2) - gzz
//                           A = (dX, dY, dW),  Q = (dX*d, dY*d, dW*d)
//                 dp[0..2] = A0*x, A0*y, A0;  dp[3..5] = A1*x, A1*y, A1;  dp[6..8] = A2*x, A2*y, A2;  dp[9..11] = Q
//               grad_depth[s][i][j] += d depth: one writer per entry, a plain load-add-store.  grad_params[s][k] += the sum of dp[k] over the
//               entries of set s in the ORDER OF THE BUILD BACKWARD above (the same bands, lanes, trees and two passes, n_params = 12).
#pragma once

#include "lerf_host_geometry.h"

namespace lerf {
namespace coords {

struct Point {
    double r, c;
};

// one (row, col) entry of a map or of a control mesh, aligned so that it moves in ONE 16-byte (double) / 8-byte (float) access
template <typename T>
struct alignas(2 * sizeof(T)) Entry {
    T r, c;
};

constexpr int kMaxParams = LERF_COORDS_MAX_PARAMS;

struct Params {
    double p[kMaxParams];
};

LERF_HD constexpr int model_params(int model) {
    return model == LERF_COORDS_HOMOGRAPHY ? 9 : model == LERF_COORDS_RADIAL ? 8 : model == LERF_COORDS_BROWN ? 21
           : model == LERF_COORDS_FISHEYE ? 17 : model == LERF_COORDS_EQUIRECT ? 13 : -1;
}

// ---- the square root and the arc tangents in + - * /, selects and bit-casts (the statement order: the comment block at the top)
LERF_HD inline double bits_to_double(int64_t b) { return __builtin_bit_cast(double, b); }
LERF_HD inline int64_t double_to_bits(double d) { return __builtin_bit_cast(int64_t, d); }

LERF_HD inline double sqrt_pm(double x) {
#pragma clang fp contract(off)
    const bool tiny = x < 2.2250738585072014e-308;                       // below 2^-1022: a subnormal (or 0, or negative)
    const double xs = tiny ? x * 3.24518553658426726783e+32 : x;         // * 2^108
    double y = bits_to_double((double_to_bits(xs) >> 1) + 0x1FF8000000000000LL);
#pragma unroll
    for (int k = 0; k < 6; ++k) y = 0.5 * (y + xs / y);
    y = tiny ? y * 5.55111512312578270212e-17 : y;                       // * 2^-54
    y = x == 0.0 ? 0.0 : y;
    y = x > 1.7976931348623157e+308 ? x : y;                             // +inf
    return x >= 0.0 ? y : __builtin_nan("");                            // x < 0 and NaN
}

LERF_HD inline double atan_pm(double x) {
#pragma clang fp contract(off)
    const double ax = x < 0.0 ? -x : x;
    const int id = ax < 0.4375 ? -1 : ax < 0.6875 ? 0 : ax < 1.1875 ? 1 : ax < 2.4375 ? 2 : 3;
    const double num = id < 0 ? ax : id == 0 ? 2.0 * ax - 1.0 : id == 1 ? ax - 1.0 : id == 2 ? ax - 1.5 : -1.0;
    const double den = id < 0 ? 1.0 : id == 0 ? 2.0 + ax : id == 1 ? ax + 1.0 : id == 2 ? 1.0 + 1.5 * ax : ax;
    const double hi = id < 0 ? 0.0 : id == 0 ? 4.63647609000806093515e-01 : id == 1 ? 7.85398163397448278999e-01
                      : id == 2 ? 9.82793723247329054082e-01 : 1.57079632679489655800e+00;
    const double lo = id < 0 ? 0.0 : id == 0 ? 2.26987774529616870924e-17 : id == 1 ? 3.06161699786838301793e-17
                      : id == 2 ? 1.39033110312309984516e-17 : 6.12323399573676603587e-17;
    const double t = num / den;
    const double z = t * t, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                      w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                      w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    double r = hi - ((t * (s1 + s2) - lo) - t);
    r = x < 0.0 ? -r : r;
    r = ax < 1.862645149230957e-09 ? x : r;                              // |x| < 2^-29: atan(x) = x to the last bit
    return x != x ? __builtin_nan("") : r;
}

LERF_HD inline double atan2_pm(double y, double x) {
#pragma clang fp contract(off)
    const double pi_hi = 3.14159265358979311600e+00, pi_lo = 1.22464679914735317723e-16, half_pi = 1.57079632679489655800e+00;
    const double a = atan_pm(y / x);
    const bool neg = y < 0.0;                                            // false for y = -0
    double r = x < 0.0 ? (neg ? (a - pi_lo) - pi_hi : (a + pi_lo) + pi_hi) : a;
    r = x == 0.0 ? (y == 0.0 ? 0.0 : neg ? -half_pi : half_pi) : r;
    return (x != x || y != y) ? __builtin_nan("") : r;
}

template <int MODEL>
LERF_HD inline Point model_point(const double* p, int i, int j) {
#pragma clang fp contract(off)
    Point q;
    if (MODEL == LERF_COORDS_HOMOGRAPHY) {
        project_unclipped(p, i, j, &q.r, &q.c);
    } else if (MODEL == LERF_COORDS_RADIAL) {
        const double cr = p[0], cc = p[1], no = p[2], ni = p[3], hr = p[4], hc = p[5], k1 = p[6], k2 = p[7];
        const double ur = ((double)i - hr) / no;
        const double uc = ((double)j - hc) / no;
        const double r2 = ur * ur + uc * uc;
        const double f = (1.0 + k1 * r2) + (k2 * r2) * r2;
        q.r = cr + (ur * f) * ni;
        q.c = cc + (uc * f) * ni;
    } else if (MODEL == LERF_COORDS_FISHEYE) {
        const double fx = p[9], fy = p[10], cx = p[11], cy = p[12], k1 = p[13], k2 = p[14], k3 = p[15], k4 = p[16];
        double x, y;
        project_unclipped(p, i, j, &y, &x);
        const double Wh = p[6] * (double)j + p[7] * (double)i + p[8];    // project_unclipped's statement
        const double r = sqrt_pm(x * x + y * y);
        const double th = atan_pm(r), th2 = th * th;
        const double thd = th * (1.0 + th2 * (k1 + th2 * (k2 + th2 * (k3 + th2 * k4))));
        const double s = r == 0.0 ? 1.0 : thd / r;
        const bool front = Wh > 0.0;                                     // false for a NaN
        q.c = front ? fx * (x * s) + cx : __builtin_nan("");
        q.r = front ? fy * (y * s) + cy : __builtin_nan("");
    } else if (MODEL == LERF_COORDS_EQUIRECT) {
        const double sx = p[9], sy = p[10], cxp = p[11], cyp = p[12];
        const double u = (double)j, v = (double)i;
        const double dx = p[0] * u + p[1] * v + p[2], dy = p[3] * u + p[4] * v + p[5], dz = p[6] * u + p[7] * v + p[8];
        const double lon = atan2_pm(dx, dz);
        const double h = sqrt_pm(dx * dx + dz * dz);
        const double lat = atan2_pm(dy, h);
        q.c = cxp + sx * lon;
        q.r = cyp + sy * lat;
    } else {
        const double fx = p[9], fy = p[10], cx = p[11], cy = p[12];
        const double k1 = p[13], k2 = p[14], p1 = p[15], p2 = p[16], k3 = p[17], k4 = p[18], k5 = p[19], k6 = p[20];
        double x, y;
        project_unclipped(p, i, j, &y, &x);
        const double r2 = x * x + y * y;
        const double rad = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)));
        const double xy = x * y;
        const double xd = (x * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * (x * x));
        const double yd = (y * rad + p1 * (r2 + 2.0 * (y * y))) + (2.0 * p2) * xy;
        q.c = fx * xd + cx;
        q.r = fy * yd + cy;
    }
    return q;
}

// ---- adjoint of model_point (the statement order: the comment block at the top of this file)
LERF_HD inline bool finite_value(double d) { return d - d == 0.0; }      // false for +-inf and NaN

template <int MODEL>
LERF_HD inline void model_point_bwd(const double* p, int i, int j, Point g, double* dp) {
#pragma clang fp contract(off)
    constexpr int NP = model_params(MODEL);
    const Point q = model_point<MODEL>(p, i, j);
    if (MODEL == LERF_COORDS_EQUIRECT) {
        const double sx = p[9], sy = p[10];
        const double u = (double)j, v = (double)i;
        const double dx = p[0] * u + p[1] * v + p[2], dy = p[3] * u + p[4] * v + p[5], dz = p[6] * u + p[7] * v + p[8];
        const double lon = atan2_pm(dx, dz);
        const double v2 = dx * dx + dz * dz;
        const double h = sqrt_pm(v2);
        const double lat = atan2_pm(dy, h);
        dp[11] = g.c;
        dp[9] = g.c * lon;
        dp[12] = g.r;
        dp[10] = g.r * lat;
        const double dlon = g.c * sx, dlat = g.r * sy;
        const double n2 = dy * dy + h * h;
        const double ddy = n2 == 0.0 ? 0.0 : (h * dlat) / n2;
        const double dh = n2 == 0.0 ? 0.0 : -((dy * dlat) / n2);
        const bool pole = h == 0.0;
        const double dv = pole ? 0.0 : dh / (2.0 * h);
        const double ddx = pole ? 0.0 : (dz * dlon) / v2 + dv * (2.0 * dx);
        const double ddz = pole ? 0.0 : -((dx * dlon) / v2) + dv * (2.0 * dz);
        dp[0] = ddx * u; dp[1] = ddx * v; dp[2] = ddx;
        dp[3] = ddy * u; dp[4] = ddy * v; dp[5] = ddy;
        dp[6] = ddz * u; dp[7] = ddz * v; dp[8] = ddz;
    } else if (MODEL == LERF_COORDS_RADIAL) {
        const double no = p[2], ni = p[3], hr = p[4], hc = p[5], k1 = p[6], k2 = p[7];
        const double ur = ((double)i - hr) / no;
        const double uc = ((double)j - hc) / no;
        const double r2 = ur * ur + uc * uc;
        const double f = (1.0 + k1 * r2) + (k2 * r2) * r2;
        dp[0] = g.r;
        dp[1] = g.c;
        dp[3] = g.r * (ur * f) + g.c * (uc * f);
        const double ar = g.r * ni, ac = g.c * ni;
        const double df = ar * ur + ac * uc;
        dp[6] = df * r2;
        dp[7] = df * (r2 * r2);
        const double dr2 = df * (k1 + (2.0 * k2) * r2);
        const double dur = ar * f + dr2 * (2.0 * ur), duc = ac * f + dr2 * (2.0 * uc);
        dp[4] = -(dur / no);
        dp[5] = -(duc / no);
        dp[2] = -((dur * ur + duc * uc) / no);
    } else {
        const double u = (double)j, v = (double)i;
        const double Wh = p[6] * u + p[7] * v + p[8];                   // project_unclipped's statement
        double dx, dy, x, y;
        if (MODEL == LERF_COORDS_HOMOGRAPHY) {
            x = q.c; y = q.r;
            dx = g.c; dy = g.r;
        } else if (MODEL == LERF_COORDS_FISHEYE) {
            const double fx = p[9], fy = p[10], k1 = p[13], k2 = p[14], k3 = p[15], k4 = p[16];
            project_unclipped(p, i, j, &y, &x);
            const double r = sqrt_pm(x * x + y * y);
            const double th = atan_pm(r), th2 = th * th;
            const double thd = th * (1.0 + th2 * (k1 + th2 * (k2 + th2 * (k3 + th2 * k4))));
            const bool centre = r == 0.0;
            const double s = centre ? 1.0 : thd / r;
            dp[9] = g.c * (x * s);
            dp[11] = g.c;
            dp[10] = g.r * (y * s);
            dp[12] = g.r;
            const double dxs = g.c * fx, dys = g.r * fy;
            const double ds = dxs * x + dys * y;
            const double dthd = centre ? 0.0 : ds / r, drs = centre ? 0.0 : -((ds * s) / r);
            const double th3 = th * th2, th5 = th3 * th2, th7 = th5 * th2, th9 = th7 * th2;
            dp[13] = dthd * th3; dp[14] = dthd * th5; dp[15] = dthd * th7; dp[16] = dthd * th9;
            const double dth = dthd * (1.0 + th2 * (3.0 * k1 + th2 * (5.0 * k2 + th2 * (7.0 * k3 + th2 * (9.0 * k4)))));
            const double dr = drs + dth / (1.0 + r * r);
            const double dv = centre ? 0.0 : dr / (2.0 * r);
            dx = dxs * s + dv * (2.0 * x);
            dy = dys * s + dv * (2.0 * y);
        } else {
            const double fx = p[9], fy = p[10];
            const double k1 = p[13], k2 = p[14], p1 = p[15], p2 = p[16], k3 = p[17], k4 = p[18], k5 = p[19], k6 = p[20];
            project_unclipped(p, i, j, &y, &x);
            const double r2 = x * x + y * y;
            const double den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6));
            const double rad = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / den;
            const double xy = x * y;
            const double a1 = r2 + 2.0 * (x * x), a2 = r2 + 2.0 * (y * y);
            const double xd = (x * rad + (2.0 * p1) * xy) + p2 * a1;
            const double yd = (y * rad + p1 * a2) + (2.0 * p2) * xy;
            dp[9] = g.c * xd;
            dp[11] = g.c;
            dp[10] = g.r * yd;
            dp[12] = g.r;
            const double dxd = g.c * fx, dyd = g.r * fy;
            dp[15] = dxd * (2.0 * xy) + dyd * a2;
            dp[16] = dxd * a1 + dyd * (2.0 * xy);
            const double drad = dxd * x + dyd * y;
            const double dnum = drad / den, dden = -((drad * rad) / den);
            const double r4 = r2 * r2, r6 = r4 * r2;
            dp[13] = dnum * r2; dp[14] = dnum * r4; dp[17] = dnum * r6;
            dp[18] = dden * r2; dp[19] = dden * r4; dp[20] = dden * r6;
            const double dr2 = (dnum * (k1 + r2 * (2.0 * k2 + r2 * (3.0 * k3))) + dden * (k4 + r2 * (2.0 * k5 + r2 * (3.0 * k6)))) +
                               (dxd * p2 + dyd * p1);
            dx = (((dxd * rad + dxd * ((2.0 * p1) * y)) + (dxd * p2) * (4.0 * x)) + dyd * ((2.0 * p2) * y)) + dr2 * (2.0 * x);
            dy = (((dyd * rad + (dyd * p1) * (4.0 * y)) + dxd * ((2.0 * p1) * x)) + dyd * ((2.0 * p2) * x)) + dr2 * (2.0 * y);
        }
        const double dX = dx / Wh, dY = dy / Wh, dWh = -((dx * x + dy * y) / Wh);
        dp[0] = dX * u; dp[1] = dX * v; dp[2] = dX;
        dp[3] = dY * u; dp[4] = dY * v; dp[5] = dY;
        dp[6] = dWh * u; dp[7] = dWh * v; dp[8] = dWh;
    }
    const bool fin = finite_value(q.r) && finite_value(q.c);
#pragma unroll
    for (int k = 0; k < NP; ++k) dp[k] = fin ? dp[k] : 0.0;             // a select: a point that is not finite contributes nothing
}

// the band a block of the build backward's pass 1 owns, and the fixed-order tree of 64 values (the host twin's form of the wave's
// shuffle tree): v[0] is the result
constexpr int kBwdCols = 64, kBwdBand = 64, kBwdWaves = 4;

inline int build_bwd_blocks(int oH, int oW) { return ((oW + kBwdCols - 1) / kBwdCols) * ((oH + kBwdBand - 1) / kBwdBand); }

inline double tree64(double* v) {
#pragma clang fp contract(off)
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] = v[l] + v[l + off];
    return v[0];
}

// ---- reproject: a pixel of view A with its depth -> its position and depth in view B (the statement order: the top of this file)
constexpr int kReprojectParams = LERF_REPROJECT_PARAMS;

struct Reprojected {
    Point q;
    double zo;
};

template <int KIND>
LERF_HD inline Reprojected reproject_point(const double* p, double depth, int i, int j) {
#pragma clang fp contract(off)
    const double x = (double)j, y = (double)i;
    const double a0 = (p[0] * x + p[1] * y) + p[2], a1 = (p[3] * x + p[4] * y) + p[5], a2 = (p[6] * x + p[7] * y) + p[8];
    double X, Y, W, zo;
    bool ok;
    if (KIND == LERF_DEPTH_Z) {
        X = a0 * depth + p[9];
        Y = a1 * depth + p[10];
        W = a2 * depth + p[11];
        zo = W;
        ok = depth > 0.0;
    } else {
        X = a0 + p[9] * depth;
        Y = a1 + p[10] * depth;
        W = a2 + p[11] * depth;
        zo = depth == 0.0 ? __builtin_inf() : W / depth;
        ok = depth >= 0.0;
    }
    ok = ok && finite_value(depth) && W > 0.0;                           // false for a NaN in depth or W
    const double nan = __builtin_nan("");
    return {{ok ? Y / W : nan, ok ? X / W : nan}, ok ? zo : nan};
}

// dp[12] and, returned, the gradient on the entry's depth
template <int KIND>
LERF_HD inline double reproject_point_bwd(const double* p, double depth, int i, int j, Point g, double gz, double* dp) {
#pragma clang fp contract(off)
    const double x = (double)j, y = (double)i;
    const double a0 = (p[0] * x + p[1] * y) + p[2], a1 = (p[3] * x + p[4] * y) + p[5], a2 = (p[6] * x + p[7] * y) + p[8];
    const Reprojected f = reproject_point<KIND>(p, depth, i, j);
    const double W = KIND == LERF_DEPTH_Z ? a2 * depth + p[11] : a2 + p[11] * depth;      // the forward's statement
    const double dX = g.c / W, dY = g.r / W, dWm = -((g.c * f.q.c + g.r * f.q.r) / W);
    const bool zf = finite_value(f.zo);
    double dW, dd, A0, A1, A2, Q0, Q1, Q2;
    if (KIND == LERF_DEPTH_Z) {
        dW = dWm + (zf ? gz : 0.0);
        dd = (dX * a0 + dY * a1) + dW * a2;
        A0 = dX * depth; A1 = dY * depth; A2 = dW * depth;
        Q0 = dX; Q1 = dY; Q2 = dW;
    } else {
        const double gzd = zf ? gz / depth : 0.0;
        const double gzz = zf ? gzd * f.zo : 0.0;
        dW = dWm + gzd;
        dd = ((dX * p[9] + dY * p[10]) + dW * p[11]) - gzz;
        A0 = dX; A1 = dY; A2 = dW;
        Q0 = dX * depth; Q1 = dY * depth; Q2 = dW * depth;
    }
    dp[0] = A0 * x; dp[1] = A0 * y; dp[2] = A0;
    dp[3] = A1 * x; dp[4] = A1 * y; dp[5] = A1;
    dp[6] = A2 * x; dp[7] = A2 * y; dp[8] = A2;
    dp[9] = Q0; dp[10] = Q1; dp[11] = Q2;
    const bool fin = finite_value(f.q.r) && finite_value(f.q.c);         // an entry that is not valid holds NaN
#pragma unroll
    for (int k = 0; k < kReprojectParams; ++k) dp[k] = fin ? dp[k] : 0.0;
    return fin ? dd : 0.0;
}

// ---- mesh: the taps of output index k along one axis of n outputs over g vertices; returns the tap count (2 or 4)
LERF_HD inline double cubic1(double x) {
#pragma clang fp contract(off)
    const double A = -0.75;
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0;
}

LERF_HD inline double cubic2(double x) {
#pragma clang fp contract(off)
    const double A = -0.75;
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A;
}

template <int INTERP>
LERF_HD inline int mesh_axis(int k, int n, int g, int idx[4], double w[4]) {
#pragma clang fp contract(off)
    const double u = n > 1 ? ((double)k * (double)(g - 1)) / (double)(n - 1) : 0.0;      // in [0, g - 1]: k in [0, n)
    const int f = (int)floor(u);
    if (INTERP == LERF_MESH_BILINEAR) {
        const int a0 = f < g - 2 ? f : g - 2;
        const double t = u - (double)a0;
        idx[0] = a0; idx[1] = a0 + 1;
        w[0] = 1.0 - t; w[1] = t;
        return 2;
    }
    const double t = u - (double)f;
    idx[0] = clampi(f - 1, 0, g - 1); idx[1] = clampi(f, 0, g - 1); idx[2] = clampi(f + 1, 0, g - 1); idx[3] = clampi(f + 2, 0, g - 1);
    w[0] = cubic2(t + 1.0); w[1] = cubic1(t); w[2] = cubic1(1.0 - t); w[3] = cubic2(2.0 - t);
    return 4;
}

template <typename TC>
LERF_HD inline Point ctrl_entry(const TC* ctrl, int gw, int a, int b) {
    const Entry<TC> e = *reinterpret_cast<const Entry<TC>*>(ctrl + 2 * ((int64_t)a * gw + b));
    return {(double)e.r, (double)e.c};
}

template <int INTERP, typename TC>
LERF_HD inline Point mesh_point(const TC* ctrl, int gh, int gw, int full_h, int full_w, int i, int j) {
#pragma clang fp contract(off)
    constexpr int nt = INTERP == LERF_MESH_BILINEAR ? 2 : 4;
    int ir[4], ic[4];
    double wr[4], wc[4];
    mesh_axis<INTERP>(i, full_h, gh, ir, wr);
    mesh_axis<INTERP>(j, full_w, gw, ic, wc);
    Point v{0.0, 0.0};
#pragma unroll
    for (int a = 0; a < nt; ++a) {
        Point s{0.0, 0.0};
#pragma unroll
        for (int b = 0; b < nt; ++b) {
            const Point e = ctrl_entry(ctrl, gw, ir[a], ic[b]);
            if (b == 0) { s.r = wc[0] * e.r; s.c = wc[0] * e.c; }
            else { s.r = s.r + wc[b] * e.r; s.c = s.c + wc[b] * e.c; }
        }
        if (a == 0) { v.r = wr[0] * s.r; v.c = wr[0] * s.c; }
        else { v.r = v.r + wr[a] * s.r; v.c = v.c + wr[a] * s.c; }
    }
    return v;
}

// Adjoint side of mesh_axis: the weight output index k puts on vertex a (clamped taps that fall on the same vertex add up, in tap
// order), 0 when no tap of k is a.  mesh_reach: a range of output indices that contains every k with a tap on a (conservative by
// one on each side; the weight decides).
template <int INTERP>
LERF_HD inline double mesh_weight_on(int k, int n, int g, int a) {
#pragma clang fp contract(off)
    int idx[4];
    double w[4];
    constexpr int nt = INTERP == LERF_MESH_BILINEAR ? 2 : 4;
    mesh_axis<INTERP>(k, n, g, idx, w);
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < nt; ++t)
        if (idx[t] == a) s = s + w[t];
    return s;
}

template <int INTERP>
LERF_HD inline void mesh_reach(int a, int n, int g, int* lo, int* hi) {
    const int K = INTERP == LERF_MESH_BILINEAR ? 1 : 2;               // a tap on a needs floor(u) in [a - K, a + K - 1]
    if (n == 1) { *lo = 0; *hi = 0; return; }
    const int64_t l = ((int64_t)(a - K) * (n - 1)) / (g - 1) - 2, h = ((int64_t)(a + K) * (n - 1)) / (g - 1) + 2;
    *lo = l < 0 ? 0 : (int)l;
    *hi = h > n - 1 ? n - 1 : (int)h;
}

// ---- compose
struct ComposeAxis {
    int i0;
    double w0, w1;
};

LERF_HD inline ComposeAxis compose_axis(double v, int n) {
#pragma clang fp contract(off)
    const double r = clip_coord(v, n - 1);
    const int f = (int)floor(r);
    ComposeAxis x;
    x.i0 = n > 1 ? (f < n - 2 ? f : n - 2) : 0;
    const double t = r - (double)x.i0;
    x.w0 = 1.0 - t;
    x.w1 = t;
    return x;
}

// READ(row, col) -> Point: entry of A; called only for taps that count
template <typename READ>
LERF_HD inline Point compose_point(double row, double col, int aH, int aW, READ read) {
#pragma clang fp contract(off)
    if (row != row || col != col) return {__builtin_nan(""), __builtin_nan("")};      // the canonical quiet NaN, whatever B held
    const ComposeAxis R = compose_axis(row, aH), Cx = compose_axis(col, aW);
    const double wr[2] = {R.w0, R.w1}, wc[2] = {Cx.w0, Cx.w1};
    Point v{0.0, 0.0};
    for (int a = 0; a < 2; ++a) {
        if (wr[a] == 0.0) continue;
        Point s{0.0, 0.0};
        for (int b = 0; b < 2; ++b) {
            if (wc[b] == 0.0) continue;
            const Point e = read(R.i0 + a, Cx.i0 + b);
            s.r = s.r + wc[b] * e.r;
            s.c = s.c + wc[b] * e.c;
        }
        v.r = v.r + wr[a] * s.r;
        v.c = v.c + wr[a] * s.c;
    }
    return v;
}

// ---- invert
LERF_HD inline bool finite_nonzero(double d) { return d != 0.0 && d - d == 0.0; }      // d - d is NaN for +-inf and NaN

// LOAD(row, col) -> Point: entry of F.  The affine guess of the u with F(u) = q from three corners of F.
template <typename LOAD>
LERF_HD inline Point invert_start(double q_r, double q_c, int fH, int fW, LOAD load) {
#pragma clang fp contract(off)
    const Point A = load(0, 0), P = load(fH - 1, 0), Q = load(0, fW - 1);
    const double nr = (double)(fH - 1), nc = (double)(fW - 1);
    const Point B{(P.r - A.r) / nr, (P.c - A.c) / nr}, Cc{(Q.r - A.r) / nc, (Q.c - A.c) / nc};
    const double det = B.r * Cc.c - B.c * Cc.r;
    if (!finite_nonzero(det)) return {nr / 2.0, nc / 2.0};
    const Point d{q_r - A.r, q_c - A.c};
    return {(d.r * Cc.c - Cc.r * d.c) / det, (B.r * d.c - B.c * d.r) / det};
}

// Newton's method on the piecewise-bilinear F from the start u0; max_iter >= 1, fH, fW >= 2.  Every pass reads the four corners
// of ONE cell of F, at indices compose_axis clamps into F.
template <typename LOAD>
LERF_HD inline Point invert_point(double q_r, double q_c, int fH, int fW, Point u0, int max_iter, double tol, LOAD load) {
#pragma clang fp contract(off)
    const Point nan2{__builtin_nan(""), __builtin_nan("")};
    Point u = u0;
    for (int k = 0; k < max_iter; ++k) {
        if (u.r != u.r || u.c != u.c) return nan2;
        const ComposeAxis R = compose_axis(u.r, fH), Cx = compose_axis(u.c, fW);
        const Point P00 = load(R.i0, Cx.i0), P01 = load(R.i0, Cx.i0 + 1), P10 = load(R.i0 + 1, Cx.i0), P11 = load(R.i0 + 1, Cx.i0 + 1);
        const Point V{R.w0 * (Cx.w0 * P00.r + Cx.w1 * P01.r) + R.w1 * (Cx.w0 * P10.r + Cx.w1 * P11.r),
                      R.w0 * (Cx.w0 * P00.c + Cx.w1 * P01.c) + R.w1 * (Cx.w0 * P10.c + Cx.w1 * P11.c)};
        const Point e{V.r - q_r, V.c - q_c};
        if (e.r != e.r || e.c != e.c) return nan2;
        const double r = clip_coord(u.r, fH - 1), c = clip_coord(u.c, fW - 1);
        if (fabs(e.r) <= tol && fabs(e.c) <= tol) return {r, c};
        const Point Jr{Cx.w0 * (P10.r - P00.r) + Cx.w1 * (P11.r - P01.r), Cx.w0 * (P10.c - P00.c) + Cx.w1 * (P11.c - P01.c)};
        const Point Jc{R.w0 * (P01.r - P00.r) + R.w1 * (P11.r - P10.r), R.w0 * (P01.c - P00.c) + R.w1 * (P11.c - P10.c)};
        const double det = Jr.r * Jc.c - Jr.c * Jc.r;
        if (!finite_nonzero(det)) return nan2;
        u.r = r - (e.r * Jc.c - Jc.r * e.c) / det;
        u.c = c - (Jr.r * e.c - Jr.c * e.r) / det;
    }
    return nan2;
}

// ---- adjoints of compose and invert (aH, aW, fH, fW >= 2: the four corners of a cell are inside the map)
struct CellJacobian {
    Point Jr, Jc;      // dV/dr, dV/dc of the bilinear patch: invert_point's statements
    bool nan;          // a NaN among the 8 values read
};

template <typename LOAD>
LERF_HD inline CellJacobian cell_jacobian(const ComposeAxis& R, const ComposeAxis& Cx, LOAD load) {
#pragma clang fp contract(off)
    const Point P00 = load(R.i0, Cx.i0), P01 = load(R.i0, Cx.i0 + 1), P10 = load(R.i0 + 1, Cx.i0), P11 = load(R.i0 + 1, Cx.i0 + 1);
    CellJacobian J;
    J.Jr = {Cx.w0 * (P10.r - P00.r) + Cx.w1 * (P11.r - P01.r), Cx.w0 * (P10.c - P00.c) + Cx.w1 * (P11.c - P01.c)};
    J.Jc = {R.w0 * (P01.r - P00.r) + R.w1 * (P11.r - P10.r), R.w0 * (P01.c - P00.c) + R.w1 * (P11.c - P10.c)};
    J.nan = P00.r != P00.r || P00.c != P00.c || P01.r != P01.r || P01.c != P01.c || P10.r != P10.r || P10.c != P10.c || P11.r != P11.r ||
            P11.c != P11.c;
    return J;
}

// ADD(row, col, dr, dc): entry (row, col) of the gradient map gains (dr, dc); called only for taps whose two weights are not 0
template <typename ADD>
LERF_HD inline void scatter_taps(const ComposeAxis& R, const ComposeAxis& Cx, Point g, ADD add) {
#pragma clang fp contract(off)
    const double wr[2] = {R.w0, R.w1}, wc[2] = {Cx.w0, Cx.w1};
    for (int a = 0; a < 2; ++a) {
        if (wr[a] == 0.0) continue;
        for (int b = 0; b < 2; ++b) {
            if (wc[b] == 0.0) continue;
            const double w = wr[a] * wc[b];
            add(R.i0 + a, Cx.i0 + b, w * g.r, w * g.c);
        }
    }
}

// returns the inner gradient (0, 0 when !inner); outer: scatter into grad_A through ADD; LOAD is called only when inner
template <typename LOAD, typename ADD>
LERF_HD inline Point compose_bwd_point(double row, double col, Point g, int aH, int aW, bool outer, bool inner, LOAD load, ADD add) {
#pragma clang fp contract(off)
    if (row != row || col != col) return {0.0, 0.0};
    const ComposeAxis R = compose_axis(row, aH), Cx = compose_axis(col, aW);
    if (outer) scatter_taps(R, Cx, g, add);
    if (!inner) return {0.0, 0.0};
    const CellJacobian J = cell_jacobian(R, Cx, load);
    const bool pass_r = row >= 0.0 && row <= (double)(aH - 1), pass_c = col >= 0.0 && col <= (double)(aW - 1);
    const double dr = J.Jr.r * g.r + J.Jr.c * g.c, dc = J.Jc.r * g.r + J.Jc.c * g.c;
    Point d{pass_r ? dr : 0.0, pass_c ? dc : 0.0};
    if (d.r != d.r) d.r = __builtin_nan("");      // the canonical quiet NaN, whatever sign and payload the sum carried
    if (d.c != d.c) d.c = __builtin_nan("");
    return d;
}

template <typename LOAD, typename ADD>
LERF_HD inline void invert_bwd_point(double r, double c, Point g, int fH, int fW, LOAD load, ADD add) {
#pragma clang fp contract(off)
    if (r != r || c != c) return;
    const ComposeAxis R = compose_axis(r, fH), Cx = compose_axis(c, fW);
    const CellJacobian J = cell_jacobian(R, Cx, load);
    if (J.nan) return;
    const double det = J.Jr.r * J.Jc.c - J.Jr.c * J.Jc.r;
    if (!finite_nonzero(det)) return;
    const Point v{-(J.Jc.c * g.r - J.Jr.c * g.c) / det, -(J.Jr.r * g.c - J.Jc.r * g.r) / det};
    scatter_taps(R, Cx, v, add);
}

// ---- invert_raster: the per-triangle and per-pixel arithmetic of the rasterising inverse (the statement order: the top of this file)
constexpr uint64_t kNoKey = ~(uint64_t)0;      // an untouched pixel
constexpr int kMaxSpan = 64;

LERF_HD inline double edge_fn(Point P, Point Q, double q_r, double q_c) {
#pragma clang fp contract(off)
    return (Q.c - P.c) * (q_r - P.r) - (Q.r - P.r) * (q_c - P.c);
}

struct TriEdges {
    double a, b, c;      // the edge functions opposite A, B, C
};

LERF_HD inline TriEdges tri_edges(Point A, Point B, Point C, bool odd, double q_r, double q_c) {
#pragma clang fp contract(off)
    TriEdges e;
    e.c = odd ? -edge_fn(B, A, q_r, q_c) : edge_fn(A, B, q_r, q_c);
    e.a = odd ? -edge_fn(C, B, q_r, q_c) : edge_fn(B, C, q_r, q_c);
    e.b = odd ? edge_fn(C, A, q_r, q_c) : -edge_fn(A, C, q_r, q_c);
    return e;
}

LERF_HD inline bool tri_inside(const TriEdges& e, double area2) {
    return area2 > 0.0 ? (e.a >= 0.0 && e.b >= 0.0 && e.c >= 0.0) : (e.a <= 0.0 && e.b <= 0.0 && e.c <= 0.0);
}

// the position in F's index space of the point with edge functions e in triangle `odd` of cell (i, j)
LERF_HD inline Point tri_value(int i, int j, bool odd, const TriEdges& e, double area2) {
#pragma clang fp contract(off)
    const double lb = e.b / area2, lc = e.c / area2;
    return odd ? Point{(double)(i + 1) - lc, (double)(j + 1) - lb} : Point{(double)i + lc, (double)j + lb};
}

LERF_HD inline float tri_depth(const TriEdges& e, double area2, float zA, float zB, float zC) {
#pragma clang fp contract(off)
    const double lb = e.b / area2, lc = e.c / area2;
    const float z = (float)((double)zA + (lb * ((double)zB - (double)zA) + lc * ((double)zC - (double)zA)));
    return z != z ? __builtin_nanf("") : z;
}

LERF_HD inline uint64_t raster_key(float z, uint32_t t) {
    const uint32_t b = __builtin_bit_cast(uint32_t, z);
    const uint32_t s = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)s << 32) | (uint64_t)t;
}

struct RasterBox {
    double area2;
    int r0, r1, c0, c1;      // the pixels of the tile the triangle may cover, inclusive
};

LERF_HD inline double min3(double a, double b, double c) { const double m = b < a ? b : a; return c < m ? c : m; }
LERF_HD inline double max3(double a, double b, double c) { const double m = b > a ? b : a; return c > m ? c : m; }

// one axis of the box: false = skipped (torn, or no pixel of the tile); the clip precedes the conversion to int
LERF_HD inline bool raster_axis(double a, double b, double c, int max_span, int first, int n, int* lo_i, int* hi_i) {
#pragma clang fp contract(off)
    double lo = ceil(min3(a, b, c)), hi = floor(max3(a, b, c));
    if ((hi - lo) + 1.0 > (double)max_span) return false;
    const double f = (double)first, l = (double)first + (double)(n - 1);
    lo = lo < f ? f : lo;
    hi = hi > l ? l : hi;
    if (lo > hi) return false;
    *lo_i = (int)lo;
    *hi_i = (int)hi;
    return true;
}

// false: the triangle is skipped.  has_depth: zA, zB, zC are tested for NaN.
LERF_HD inline bool raster_setup(Point A, Point B, Point C, bool has_depth, float zA, float zB, float zC, int orient, int max_span, int i0, int j0,
                                 int oH, int oW, RasterBox* box) {
#pragma clang fp contract(off)
    if (!(finite_value(A.r) && finite_value(A.c) && finite_value(B.r) && finite_value(B.c) && finite_value(C.r) && finite_value(C.c))) return false;
    if (has_depth && (zA != zA || zB != zB || zC != zC)) return false;
    const double area2 = edge_fn(A, B, C.r, C.c);
    if (!finite_nonzero(area2)) return false;
    if ((orient > 0 && area2 < 0.0) || (orient < 0 && area2 > 0.0)) return false;
    box->area2 = area2;
    return raster_axis(A.r, B.r, C.r, max_span, i0, oH, &box->r0, &box->r1) && raster_axis(A.c, B.c, C.c, max_span, j0, oW, &box->c0, &box->c1);
}

// Both triangles of cell (i, j) into the tile.  LOAD(row, col) -> Point of F; depth: dense [fH][fW] float32 or null;
// MINKEY(index, key): keys[index] = min(keys[index], key), index = (row - i0)*oW + (col - j0) inside [oH][oW] by the clipped box.
template <typename LOAD, typename MINKEY>
LERF_HD inline void raster_cell(int i, int j, int fW, LOAD load, const float* depth, int orient, int max_span, int i0, int j0, int oH, int oW,
                                MINKEY minkey) {
#pragma clang fp contract(off)
    const Point P[4] = {load(i, j), load(i, j + 1), load(i + 1, j), load(i + 1, j + 1)};
    float Z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (depth) {
        const float* d = depth + (int64_t)i * fW + j;
        Z[0] = d[0]; Z[1] = d[1]; Z[2] = d[fW]; Z[3] = d[fW + 1];
    }
    const uint32_t t0 = 2u * ((uint32_t)i * (uint32_t)(fW - 1) + (uint32_t)j);
    for (int odd = 0; odd < 2; ++odd) {
        const int a = odd ? 3 : 0, b = odd ? 2 : 1, c = odd ? 1 : 2;
        const Point A = P[a], B = P[b], C = P[c];
        RasterBox box;
        if (!raster_setup(A, B, C, depth != nullptr, Z[a], Z[b], Z[c], orient, max_span, i0, j0, oH, oW, &box)) continue;
        for (int r = box.r0; r <= box.r1; ++r)
            for (int q = box.c0; q <= box.c1; ++q) {
                const TriEdges e = tri_edges(A, B, C, odd != 0, (double)r, (double)q);
                if (!tri_inside(e, box.area2)) continue;
                const float z = depth ? tri_depth(e, box.area2, Z[a], Z[b], Z[c]) : 0.0f;
                minkey((int64_t)(r - i0) * oW + (q - j0), raster_key(z, t0 + (uint32_t)odd));
            }
    }
}

// the entry of the inverse a winning key stands for
template <typename LOAD>
LERF_HD inline Point raster_resolve(uint64_t key, int fW, double q_r, double q_c, LOAD load) {
#pragma clang fp contract(off)
    if (key == kNoKey) return {__builtin_nan(""), __builtin_nan("")};
    const uint32_t t = (uint32_t)key, cell = t >> 1;
    const bool odd = (t & 1u) != 0;
    const int i = (int)(cell / (uint32_t)(fW - 1)), j = (int)(cell % (uint32_t)(fW - 1));
    const Point A = odd ? load(i + 1, j + 1) : load(i, j), B = odd ? load(i + 1, j) : load(i, j + 1), C = odd ? load(i, j + 1) : load(i + 1, j);
    const double area2 = edge_fn(A, B, C.r, C.c);
    return tri_value(i, j, odd, tri_edges(A, B, C, odd, q_r, q_c), area2);
}

// ---- trimesh: an INDEXED triangle mesh drawn into a map (the statement order: the top of this file).  The per-pixel functions are
// invert_raster's (edge_fn, tri_inside, tri_depth, raster_key); what is new is the edge rule by vertex index, the optional tear rule,
// the w test, the interpolated attribute and the item tiles of the device's hot path.
constexpr int kTileRows = 4, kTileCols = 16;      // an item tile of the key plane: a wave's 64 pixels, four runs of 128 contiguous bytes of keys
constexpr int kMaxTriSpan = 65536;

// all three indices inside [0, n): ONE unsigned compare each, so a negative index is a large one
LERF_HD inline bool tri_index_ok(int32_t a, int32_t b, int32_t c, int n) {
    return (uint32_t)a < (uint32_t)n && (uint32_t)b < (uint32_t)n && (uint32_t)c < (uint32_t)n;
}

// tri_edges with `odd` generalised: every directed edge P -> Q of A -> B -> C -> A is evaluated from its lower vertex index
LERF_HD inline TriEdges tri_edges_indexed(Point A, Point B, Point C, int32_t ia, int32_t ib, int32_t ic, double q_r, double q_c) {
#pragma clang fp contract(off)
    TriEdges e;
    e.c = ia < ib ? edge_fn(A, B, q_r, q_c) : -edge_fn(B, A, q_r, q_c);
    e.a = ib < ic ? edge_fn(B, C, q_r, q_c) : -edge_fn(C, B, q_r, q_c);
    e.b = ic < ia ? edge_fn(C, A, q_r, q_c) : -edge_fn(A, C, q_r, q_c);
    return e;
}

// raster_axis with the tear rule optional (max_span == 0: none)
LERF_HD inline bool tri_axis(double a, double b, double c, int max_span, int first, int n, int* lo_i, int* hi_i) {
#pragma clang fp contract(off)
    double lo = ceil(min3(a, b, c)), hi = floor(max3(a, b, c));
    if (max_span > 0 && (hi - lo) + 1.0 > (double)max_span) return false;
    const double f = (double)first, l = (double)first + (double)(n - 1);
    lo = lo < f ? f : lo;
    hi = hi > l ? l : hi;
    if (lo > hi) return false;
    *lo_i = (int)lo;
    *hi_i = (int)hi;
    return true;
}

// one face with its vertices read: what the set-up, the pixels and the resolve share
struct TriFace {
    Point A, B, C;
    int32_t ia, ib, ic;      // indices into pos: the edge rule
    float zA, zB, zC;        // +0.0f without depth
};

// false: the face is skipped.  raster_setup's tests with the w test after the depths and the tear rule optional
LERF_HD inline bool tri_setup(const TriFace& t, bool has_depth, bool has_w, double wA, double wB, double wC, int orient, int max_span, int i0, int j0,
                              int oH, int oW, RasterBox* box) {
#pragma clang fp contract(off)
    if (!(finite_value(t.A.r) && finite_value(t.A.c) && finite_value(t.B.r) && finite_value(t.B.c) && finite_value(t.C.r) && finite_value(t.C.c)))
        return false;
    if (has_depth && (t.zA != t.zA || t.zB != t.zB || t.zC != t.zC)) return false;
    if (has_w && !(finite_value(wA) && finite_value(wB) && finite_value(wC) && wA > 0.0 && wB > 0.0 && wC > 0.0)) return false;
    const double area2 = edge_fn(t.A, t.B, t.C.r, t.C.c);
    if (!finite_nonzero(area2)) return false;
    if ((orient > 0 && area2 < 0.0) || (orient < 0 && area2 > 0.0)) return false;
    box->area2 = area2;
    return tri_axis(t.A.r, t.B.r, t.C.r, max_span, i0, oH, &box->r0, &box->r1) && tri_axis(t.A.c, t.B.c, t.C.c, max_span, j0, oW, &box->c0, &box->c1);
}

// the item tiles a clipped box touches: tiles are aligned to the plane's own rows and columns (relative to the tile origin (i0, j0))
struct TriTiles {
    int tr0, tc0, ntr, ntc;
};

LERF_HD inline TriTiles tri_tiles(const RasterBox& box, int i0, int j0) {
    TriTiles t;
    t.tr0 = (box.r0 - i0) / kTileRows;
    t.tc0 = (box.c0 - j0) / kTileCols;
    t.ntr = (box.r1 - i0) / kTileRows - t.tr0 + 1;
    t.ntc = (box.c1 - j0) / kTileCols - t.tc0 + 1;
    return t;
}

// the most item tiles one face can have: the tiles of the plane, or of a box max_span wide where that is fewer (sizes only)
inline int64_t tri_axis_tiles(int n, int max_span, int tile) {
    const int64_t plane = ((int64_t)n + tile - 1) / tile;
    const int64_t span = max_span > 0 ? ((int64_t)max_span + tile - 2) / tile + 1 : plane;
    return span < plane ? span : plane;
}

// pixel (r, q) of the frame against one face that passed the set-up: MINKEY(index, key) as in raster_cell
template <typename MINKEY>
LERF_HD inline void tri_pixel(const TriFace& t, const RasterBox& box, bool has_depth, uint32_t f, int r, int q, int i0, int j0, int oW, MINKEY minkey) {
#pragma clang fp contract(off)
    const TriEdges e = tri_edges_indexed(t.A, t.B, t.C, t.ia, t.ib, t.ic, (double)r, (double)q);
    if (!tri_inside(e, box.area2)) return;
    const float z = has_depth ? tri_depth(e, box.area2, t.zA, t.zB, t.zC) : 0.0f;
    minkey((int64_t)(r - i0) * oW + (q - j0), raster_key(z, f));
}

// the float a key's high word stands for: the exact inverse of raster_key's sortable()
LERF_HD inline float key_depth(uint64_t key) {
    const uint32_t s = (uint32_t)(key >> 32);
    const uint32_t b = (s & 0x80000000u) ? (s & 0x7fffffffu) : ~s;
    return __builtin_bit_cast(float, b);
}

// the attribute at pixel q of the face whose attributes are aA, aB, aC; has_w: perspective-correct with the vertices' w (a float32 w promoted exactly)
LERF_HD inline Point tri_attr(const TriFace& t, Point aA, Point aB, Point aC, bool has_w, double wA, double wB, double wC, double q_r, double q_c) {
#pragma clang fp contract(off)
    const double area2 = edge_fn(t.A, t.B, t.C.r, t.C.c);
    const TriEdges e = tri_edges_indexed(t.A, t.B, t.C, t.ia, t.ib, t.ic, q_r, q_c);
    const double lb = e.b / area2, lc = e.c / area2;
    if (!has_w) return {aA.r + (lb * (aB.r - aA.r) + lc * (aC.r - aA.r)), aA.c + (lb * (aB.c - aA.c) + lc * (aC.c - aA.c))};
    const double ia = 1.0 / wA, ib = 1.0 / wB, ic = 1.0 / wC;
    const double d = ia + (lb * (ib - ia) + lc * (ic - ia));
    const double nr = aA.r * ia + (lb * (aB.r * ib - aA.r * ia) + lc * (aC.r * ic - aA.r * ia));
    const double nc = aA.c * ia + (lb * (aB.c * ib - aA.c * ia) + lc * (aC.c * ic - aA.c * ia));
    return {nr / d, nc / d};
}

// ---- trimesh backward: the adjoint of tri_attr at fixed visibility (the statement order: the top of this file)
constexpr int kTriBwdWaves = 4;       // waves of the face pass: thread t = 64 r + l owns lane pixel l of the item tiles r, r + 4, ...
constexpr int kTriBwdTerms = 15;      // a face's terms: [corner A, B, C][attr.r, attr.c, pos.r, pos.c, w]

// the constant gradients of the barycentrics with respect to the pixel: (d l_k / d q.r, d l_k / d q.c)
struct TriGrads {
    Point a, b, c;
};

LERF_HD inline TriGrads tri_grads(const TriFace& t, double area2) {
#pragma clang fp contract(off)
    TriGrads G;
    G.a = {(t.C.c - t.B.c) / area2, -((t.C.r - t.B.r) / area2)};
    G.b = {(t.A.c - t.C.c) / area2, -((t.A.r - t.C.r) / area2)};
    G.c = {(t.B.c - t.A.c) / area2, -((t.B.r - t.A.r) / area2)};
    return G;
}

// the terms pixel q adds to the sums of the face that won it, upstream g: d[5 k + 0, 1] for attr of corner k, with w also d[5 k + 2, 3]
// for pos and d[5 k + 4] for w; without w only the six attr terms are written (the pos terms come from their SUMS: tri_face_terms)
template <bool HAS_W>
LERF_HD inline void tri_attr_bwd(const TriFace& t, const TriGrads& G, Point aA, Point aB, Point aC, double wA, double wB, double wC, double q_r,
                                 double q_c, Point g, double* d) {
#pragma clang fp contract(off)
    const double area2 = edge_fn(t.A, t.B, t.C.r, t.C.c);
    const TriEdges e = tri_edges_indexed(t.A, t.B, t.C, t.ia, t.ib, t.ic, q_r, q_c);
    const double lb = e.b / area2, lc = e.c / area2;
    const double la = (1.0 - lb) - lc;
    if (!HAS_W) {
        d[0] = la * g.r; d[1] = la * g.c;
        d[5] = lb * g.r; d[6] = lb * g.c;
        d[10] = lc * g.r; d[11] = lc * g.c;
        return;
    }
    const double ia = 1.0 / wA, ib = 1.0 / wB, ic = 1.0 / wC;
    const double dd = ia + (lb * (ib - ia) + lc * (ic - ia));
    const double nr = aA.r * ia + (lb * (aB.r * ib - aA.r * ia) + lc * (aC.r * ic - aA.r * ia));
    const double nc = aA.c * ia + (lb * (aB.c * ib - aA.c * ia) + lc * (aC.c * ic - aA.c * ia));
    const double ur = nr / dd, uc = nc / dd;                                                      // tri_attr's value
    const double ma = (la * ia) / dd, mb = (lb * ib) / dd, mc = (lc * ic) / dd;
    const double ha = ((aA.r - ur) * g.r + (aA.c - uc) * g.c) * ia;
    const double hb = ((aB.r - ur) * g.r + (aB.c - uc) * g.c) * ib;
    const double hc = ((aC.r - ur) * g.r + (aC.c - uc) * g.c) * ic;
    const double vr = ((ha * G.a.r + hb * G.b.r) + hc * G.c.r) / dd;                              // J(q)^T g
    const double vc = ((ha * G.a.c + hb * G.b.c) + hc * G.c.c) / dd;
    d[0] = ma * g.r; d[1] = ma * g.c; d[2] = -(la * vr); d[3] = -(la * vc); d[4] = -(ma * ha);
    d[5] = mb * g.r; d[6] = mb * g.c; d[7] = -(lb * vr); d[8] = -(lb * vc); d[9] = -(mb * hb);
    d[10] = mc * g.r; d[11] = mc * g.c; d[12] = -(lc * vr); d[13] = -(lc * vc); d[14] = -(mc * hc);
}

// the face's 15 terms T from its reduced sums S (both [corner][5]); without w the pos terms are -J^T S_m, J the face's constant Jacobian
LERF_HD inline void tri_face_terms(const TriGrads& G, Point aA, Point aB, Point aC, bool has_w, const double* S, double* T) {
#pragma clang fp contract(off)
    const double Jrr = (aA.r * G.a.r + aB.r * G.b.r) + aC.r * G.c.r, Jrc = (aA.r * G.a.c + aB.r * G.b.c) + aC.r * G.c.c;
    const double Jcr = (aA.c * G.a.r + aB.c * G.b.r) + aC.c * G.c.r, Jcc = (aA.c * G.a.c + aB.c * G.b.c) + aC.c * G.c.c;
    for (int m = 0; m < 3; ++m) {
        const double sr = S[5 * m], sc = S[5 * m + 1];
        T[5 * m] = sr;
        T[5 * m + 1] = sc;
        T[5 * m + 2] = has_w ? S[5 * m + 2] : -(Jrr * sr + Jcr * sc);
        T[5 * m + 3] = has_w ? S[5 * m + 3] : -(Jrc * sr + Jcc * sc);
        T[5 * m + 4] = has_w ? S[5 * m + 4] : 0.0;
    }
    for (int k = 0; k < kTriBwdTerms; ++k)
        if (T[k] != T[k]) T[k] = __builtin_nan("");      // the canonical quiet NaN: the host and the device agree on its bits
}

// the sums of one thread of the face pass: wave slot r, lane l (pixel lr = l / 16, lc = l % 16 of an item tile), over the item tiles
// k = r, r + kTriBwdWaves, ... of the face's clipped box, in ascending k, into acc (NS values: 15 with w, the 6 attr sums without,
// in the order of the terms).  A pixel adds only when it lies in the box, its key is not all ones and the key's low word is f; any
// other pixel forms no address in gout.  keys, gout: the planes of the face's set, [oH][oW] and [oH][oW][2].
template <bool HAS_W>
LERF_HD inline void tri_bwd_thread(const TriFace& t, const RasterBox& box, const TriGrads& G, Point aA, Point aB, Point aC, double wA, double wB,
                                   double wC, uint32_t f, int i0, int j0, int oW, const uint64_t* keys, const double* gout, int r, int l, double* acc) {
#pragma clang fp contract(off)
    constexpr int NS = HAS_W ? kTriBwdTerms : 6;
    const TriTiles tt = tri_tiles(box, i0, j0);
    const uint32_t n = (uint32_t)tt.ntr * (uint32_t)tt.ntc;
    const int lr = l / kTileCols, lc = l % kTileCols;
    for (uint32_t k = (uint32_t)r; k < n; k += (uint32_t)kTriBwdWaves) {
        const int rr = (tt.tr0 + (int)(k / (uint32_t)tt.ntc)) * kTileRows + lr, qq = (tt.tc0 + (int)(k % (uint32_t)tt.ntc)) * kTileCols + lc;
        if (rr < box.r0 - i0 || rr > box.r1 - i0 || qq < box.c0 - j0 || qq > box.c1 - j0) continue;
        const int64_t e = (int64_t)rr * oW + qq;
        const uint64_t key = keys[e];
        if (key == kNoKey || (uint32_t)key != f) continue;
        const Entry<double> g = *reinterpret_cast<const Entry<double>*>(gout + 2 * e);
        double d[kTriBwdTerms];
        tri_attr_bwd<HAS_W>(t, G, aA, aB, aC, wA, wB, wC, (double)(i0 + rr), (double)(j0 + qq), Point{g.r, g.c}, d);
        if (HAS_W) {
#pragma unroll
            for (int k2 = 0; k2 < NS; ++k2) acc[k2] = acc[k2] + d[k2];
        } else {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                acc[2 * m] = acc[2 * m] + d[5 * m];
                acc[2 * m + 1] = acc[2 * m + 1] + d[5 * m + 1];
            }
        }
    }
}

}  // namespace coords
}  // namespace lerf
