// box_body.inc - the body of search3_box_kernel / search3_box_single_kernel (corr_kernels.hip), textually included
// into both: the two kernels differ only in how their arguments arrive (two SearchJob structs addressed through the
// kernel-argument segment vs plain by-value arguments), and routing the body through a function call boundary
// instead cost the stepped instantiations 22 more spilled VGPRs.  In scope at the point of inclusion: template
// parameters COUNT, STEP, TR, WIDE and the names p, img1, img2, stats1, istats1, istats2, range, contenders, out, counters,
// out_score, declined, whole_list.
// This file has two sections.  With BOX_STEP_SECTION defined it is ONE STEP OF THE WALK, which the kernels' body below includes
// into each of its loops: the stepped plans' one loop, and the lean plan's two - the steps nobody folded, where `step` is
// wave-uniform (scalar addresses, a scalar record code), and the folded pairs, where it is the lane's own.  (As a lambda called
// from the three places the step cost the stepped instantiations 300 bytes of scratch; in a file of its own it would escape the
// hash of the kernels' sources that the committed counter profiles carry.)  In scope there: everything the body has set up before
// its walk, and `step`.
#ifdef BOX_STEP_SECTION
            const int dx = mnx + step; // displacement along the lanes (x; y when TR)
            const bool mx = has && (uint32_t)(dx - lou) < wu;
            // first plane offset of this lane's candidates at this step, and the planes the wave needs for it
            int bl = lov, s0 = ws0, n = wn;
            if (wave_step) {
                if (!__builtin_amdgcn_ballot_w64(mx)) continue; // nobody searches this step
                // the wave's window at this step, from the table settled in setup (lane `step` holds it; step 64: step_last)
                const uint32_t tw = step < STEP_TABLE ? (uint32_t)__builtin_amdgcn_readlane((int)step_tbl, step) : step_last;
                s0 = ws0 + (int)(tw & 0xFFFFu);
                n = (int)(tw >> 16);
                if (COUNT && stepped && mx) {
                    // (the candidate counter tests every plane's membership - and, while it is at it, that the table's window
                    // holds this lane's stripes: a bracket that missed would show up as a wildly wrong candidate count)
                    bl = step_first_plane(dx);
                    if (bl < dy0 + s0 || bl + WV > dy0 + s0 + n) bracket_missed = true;
                }
            }
            uint32_t raw[NDW];
            const uint8_t *pIS = bIS + step * 8;
            int dyb = dy0; // displacement (across the planes) of plane index 0 of this step's groups
            int first = 0; // plane index of the wave's first plane at this step
            if constexpr (STEP) {
                // the tall copy: 24 bytes from the dword that holds this wave's first row at this step; the planes then
                // start at byte `first` = 0..3 of it, and the statistics rows / displacements are counted from there
                const int off = (int)w + s0;
                first = off & 3;
                const uint32_t *pc = bCOL + step * (int)PD + (off >> 2);
#pragma unroll
                for (int k = 0; k < NDW; k++) raw[k] = pc[k];
                pIS += (s0 - first) * (ISP * 8);
                dyb = dy0 + s0 - first;
            } else {
                const uint4 r4 = *reinterpret_cast<const uint4 *>(bB16 + step * 16);
                raw[0] = r4.x;
                raw[1] = r4.y;
                raw[2] = r4.z;
                raw[3] = r4.w;
                raw[4] = *reinterpret_cast<const uint32_t *>(bB4 + step * TAIL_BYTES);
            }
            // one group of planes: s = S0 .. S0 + N - 1 (dy = dyb + s), all independent until the rare branch
            auto group = [&](auto s0_tag, auto n_tag) {
                constexpr int S0 = decltype(s0_tag)::value, N = decltype(n_tag)::value;
                int num[N];
                float rs[N]; // lean plan: 1 / stdev of the plane's candidate (0: none); stepped plan: the stdev (+inf: none)
#pragma unroll
                for (int q = 0; q < N; q++) {
                    const int s = S0 + q, sh = s & 3, o = s >> 2;
                    const uint2 is2 = *reinterpret_cast<const uint2 *>(pIS + s * (ISP * 8));
                    uint32_t c = __builtin_amdgcn_udot4(a[sh][0], raw[o], 0u, false);
                    c = __builtin_amdgcn_udot4(a[sh][1], raw[o + 1], c, false);
                    c = __builtin_amdgcn_udot4(a[sh][2], raw[o + 2], c, false);
                    if (sh >= 2) c = __builtin_amdgcn_udot4(a[sh][3], raw[o + 3 < NDW ? o + 3 : NDW - 1], c, false);
                    const uint32_t pre = wave_prefix_sum(c);
                    const uint32_t s12 = pre - (uint32_t)__builtin_amdgcn_ds_bpermute(idx_lo, (int)pre);
                    num[q] = __mul24((int)s12, KERNEL_POINT_COUNT) + __mul24((int)s1, (int)is2.x);
                    rs[q] = __uint_as_float(is2.y);
                }
                // one branch for the group: the largest margin decides - lean plan fl(x - T) against -2 D, stepped plan
                // (float)N - limk sd2 against 0 (see record()); a hit is re-tested below against the state of that moment.
                float mg[N];
#pragma unroll
                for (int q = 0; q < N; q++) mg[q] = RS ? __builtin_fmaf((float)num[q], rs[q], -T) : __builtin_fmaf(-limk, rs[q], (float)num[q]);
                float margin = mg[0];
#pragma unroll
                for (int q = 1; q < N; q++) margin = fmaxf(margin, mg[q]);
                const float mlo = RS ? M : 0.0f;
                if (COUNT) {
#pragma unroll
                    for (int q = 0; q < N; q++)
                        if (mx && (uint32_t)(dyb + S0 + q - bl) < wv && (RS ? rs[q] > 0.0f : rs[q] < __builtin_inff())) evaluated++;
                }
                if (margin >= mlo && !(dbg & 64)) {
                    // (stepped lines: the lane's own first plane at this step, needed only here)
                    // (behind an opaque copy of dx: the compiler otherwise evaluates the six f64 operations ahead of the branch,
                    // in every step)
                    // Where the table's window is exactly one pixel's stripes (n == WV) every searching lane's first plane IS the
                    // window's - the bracket holds them all - and nothing is evaluated: the rule for parallel lines, except where
                    // they pass a row.
                    if (STEP && !COUNT && wave_step && stepped && mx) {
                        bl = dy0 + s0;
                        if (n != WV) {
                            int dxl = dx;
                            asm volatile("" : "+s"(dxl));
                            bl = step_first_plane(dxl);
                        }
                    }
                    if (STEP && LOOSE_OK && wave_loose) {
                        // A wave with loose lanes (rare: lines within an ulp below a row 2^k): one plane at a time, in a loop
                        // - this path exists once per group, not once per plane, and the usual one below stays as it was.
                        // For a loose lane the reference's own expression (mod.rs:424-429) says which stripe lies on the
                        // plane's row at this step; none: the row its stripes skip here.
#pragma nounroll
                        for (int j = 0; j < N; j++) {
                            float rsj = rs[0];
                            int numj = num[0];
#pragma unroll
                            for (int q = 1; q < N; q++) {
                                rsj = j == q ? rs[q] : rsj;
                                numj = j == q ? num[q] : numj;
                            }
                            const int dy = dyb + S0 + j;
                            if (mx && (uint32_t)(dy - bl) < wv && rsj < __builtin_inff() && (float)numj >= limk * rsj) { // (stepped plan: rs IS the stdev)
                                uint32_t stripe = (uint32_t)(dy - bl);
                                if (wv == (uint32_t)WV + 1u) { // (a loose lane: six planes)
                                    stripe = 0xFFFFFFFFu;
                                    const uint32_t ci = (uint32_t)((TR ? (int)y : xi) + dx), crow = (uint32_t)((TR ? xi : (int)y) + dy);
                                    for (int off = cs; off >= -cs; off--) {
                                        const CandXY co = candidate_xy(e, ci, off);
                                        if ((TR ? co.x : co.y) == crow) stripe = (uint32_t)(off + cs);
                                    }
                                }
                                const int dmaj = (TR ? (int)y : xi) + dx - (int)r0; // position along the line (stepped lanes: major_x != TR)
                                const float rr = __builtin_amdgcn_rcpf(rsj);
                                if (stripe != 0xFFFFFFFFu)
                                    record(__builtin_fmaf((float)numj, rr, -T) > 0.0f, __builtin_fmaf((float)numj, rr, D), (stripe << 11) | (uint32_t)dmaj);
                            }
                        }
                        return;
                    }
                    // Planes from the middle of the group outwards: every record raises the bound, and the stripe through
                    // the predicted position is where the best match usually is - once it is in, its neighbours
                    // (typically 0.6 .. 0.9 against ~1) fail the re-test and their record bodies are skipped.  The
                    // order is free: the contender list is unordered and re-evaluated exactly.
#pragma unroll
                    for (int qi = 0; qi < N; qi++) {
                        const int q = (N - 1) / 2 + ((qi & 1) ? (qi + 1) / 2 : -(qi / 2)); // m, m+1, m-1, m+2, ...
                        const int dy = dyb + S0 + q; // displacement across the planes (y; x when TR)
                        // (the plane's own pre-screen margin first - one compare; it was taken with a T that has only risen
                        // since, so nothing that passes the test below is missed.  Lean plan: the first plane's margin IS the
                        // test - nothing was recorded since.)
                        const float mgc = qi == 0 ? mg[q] : __builtin_fmaf((float)num[q], rs[q], -T); // (lean plan)
                        if (mg[q] >= mlo && mx && (uint32_t)(dy - bl) < wv &&
                            (RS ? mgc >= M : (rs[q] < __builtin_inff() && (float)num[q] >= limk * rs[q]))) {
                            if (RS) {
                                record(mgc > 0.0f, __builtin_fmaf((float)num[q], rs[q], D), ((uint32_t)(S0 + q) << 7) | (uint32_t)step);
                            } else {
                                // back to image axes: candidate (x + ddx, y + ddy), stripe origin (ox, oy)
                                const int ddx = TR ? dy : dx, ddy = TR ? dx : dy, ox = TR ? bl : lox, oy = TR ? loy : bl;
                                const uint32_t code = major_x ? ((uint32_t)(ddy - oy) << 11) | (uint32_t)(xi + ddx - (int)r0)
                                                              : ((uint32_t)(ddx - ox) << 11) | (uint32_t)((int)y + ddy - (int)r0);
                                const float rr = __builtin_amdgcn_rcpf(rs[q]);
                                record(__builtin_fmaf((float)num[q], rr, -T) > 0.0f, __builtin_fmaf((float)num[q], rr, D), code);
                            }
                        }
                    }
                }
            };
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, 1>;
            using I2 = std::integral_constant<int, 2>;
            using I3 = std::integral_constant<int, 3>;
            using I4 = std::integral_constant<int, 4>;
            using I5 = std::integral_constant<int, 5>;
            if (!STEP) { // rectangles only: the workgroup's planes 0..4, and 5..8 when its box is taller
                group(I0{}, I5{});
                if (NPL > 5) group(I5{}, I4{});
                continue;
            }
            if constexpr (STEP) {
                using I6 = std::integral_constant<int, 6>;
                using I7 = std::integral_constant<int, 7>;
                using I8 = std::integral_constant<int, 8>;
                using I9 = std::integral_constant<int, 9>;
                using I10 = std::integral_constant<int, 10>;
                using I11 = std::integral_constant<int, 11>;
                using I12 = std::integral_constant<int, 12>;
                using I13 = std::integral_constant<int, 13>;
                // planes are register-indexed, so the window position selects an instantiation: five planes from
                // `first` in one interleaved group (n >= 5: every pixel has at least five stripes), ...
                if (n == 6) { // (one row straddled inside a five-stripe window: six interleaved planes, not five and one alone)
                    switch (first) {
                    case 0: group(I0{}, I6{}); break;
                    case 1: group(I1{}, I6{}); break;
                    case 2: group(I2{}, I6{}); break;
                    default: group(I3{}, I6{}); break;
                    }
                    continue;
                }
                switch (first) {
                case 0: group(I0{}, I5{}); break;
                case 1: group(I1{}, I5{}); break;
                case 2: group(I2{}, I5{}); break;
                default: group(I3{}, I5{}); break;
                }
                // ... then one more interleaved group where three or more remain (nine stripes), the rest singly
                // (five stripes whose lines step inside the box).  first + n <= 3 + S3_MAXH = 14 planes in 24 bytes.
                int sx = first + 5, left = n - 5;
                if (left >= 5) {
                    switch (sx) {
                    case 5: group(I5{}, I5{}); break;
                    case 6: group(I6{}, I5{}); break;
                    case 7: group(I7{}, I5{}); break;
                    default: group(I8{}, I5{}); break;
                    }
                    sx += 5;
                    left -= 5;
                } else if (left >= 3) {
                    const bool four = left == 4;
                    switch (sx) {
                    case 5: four ? group(I5{}, I4{}) : group(I5{}, I3{}); break;
                    case 6: four ? group(I6{}, I4{}) : group(I6{}, I3{}); break;
                    case 7: four ? group(I7{}, I4{}) : group(I7{}, I3{}); break;
                    default: four ? group(I8{}, I4{}) : group(I8{}, I3{}); break;
                    }
                    sx += four ? 4 : 3;
                    left = 0;
                }
                for (; left > 0; left--, sx++) {
                    switch (sx) {
                    case 5: group(I5{}, I1{}); break;
                    case 6: group(I6{}, I1{}); break;
                    case 7: group(I7{}, I1{}); break;
                    case 8: group(I8{}, I1{}); break;
                    case 9: group(I9{}, I1{}); break;
                    case 10: group(I10{}, I1{}); break;
                    case 11: group(I11{}, I1{}); break;
                    case 12: group(I12{}, I1{}); break;
                    default: group(I13{}, I1{}); break;
                    }
                }
            }
#else // ---- the kernels' body ----------------------------------------------------------------------------------------
    // (CorrParams::debug switches parts of the kernel off for the ablation scripts; only -DCVHIP_ABLATIONS builds ever set it,
    // and only they pay for looking at it - in the walk that was a scalar load and a test per step)
#ifdef CVHIP_ABLATIONS
    const int dbg = p.debug;
#else
    constexpr int dbg = 0;
#endif
    // (loose lanes - below - are walked by the instantiations that do not count candidates; ablation builds: switch bit 128 lets
    // the counting ones walk them too, for the decline statistics of scripts/_diag_declined.sh - their counts are then off)
    const bool LOOSE_OK = !COUNT || (dbg & 128);
    using Plan = S3Plan<STEP, WIDE>;
    // The staged candidate statistics carry 1 / stdev in the lean plan - a record then costs no quarter-rate v_rcp_f32 - and the
    // stdev itself in the stepped plan: its sheared boxes stage several times the cells the walk ever touches (60 degrees: the
    // reciprocals at staging cost 0.5 ms of a 7.9 ms step).
    constexpr bool RS = !STEP;
    constexpr uint32_t NO_CAND = RS ? 0u : 0x7F800000u;
    constexpr int S3_MAXH = Plan::MAXH, NDW = Plan::NDW, S3_B16_OFF = Plan::B16_OFF, S3_TAIL_OFF = Plan::TAIL_OFF,
                  TAIL_BYTES = Plan::TAIL_BYTES;
    // The lean instantiation stages 4 row-shifted copies of 20 bytes per target line in static LDS (S3Plan<false>).
    // The stepped instantiation (any line slope) stages ONE tall copy in dynamic LDS: PD dwords per line - every row
    // the workgroup's sheared displacement box can touch - and a wave reads its 24 bytes per step at the dword offset
    // its lines have reached; the candidate statistics follow, SH rows of S3_COLS cells (sizes from the host:
    // CorrParams::box_pd / box_sh; a workgroup whose box needs more declines).
    __shared__ __attribute__((aligned(16))) uint8_t lds_static[STEP ? 16 : Plan::LDS_BYTES];
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn_lds[];
    uint8_t *const lds = STEP ? dyn_lds : lds_static;
    const uint32_t PD = STEP ? p.box_pd : 0u;
    // lines staged per workgroup and cells per statistics row: the stepped plan keeps both below the lean plan's 128 -
    // its boxes are at most 33 steps wide - so that the rows a steep line needs still leave room for 4-5 workgroups per CU
    constexpr int LN = Plan::LINES, ISP = Plan::ISP;
    const int S3_IS_OFF = STEP ? (int)(LN * PD * 4u) : Plan::IS_OFF;
    __shared__ int bb[7]; // min dx, min dy, max dx, max dy, max candidates of one pixel, 1 = some pixel is not a rectangle,
                          // (stepped) the most planes one wave can need at one step

    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const TileId tid = xcd_tile();
    const int U0 = (TR ? (int)p.row0 : 0) + (int)tid.x * S3_OUT;
    const int uc = U0 - 6 + (int)lane;        // u coordinate of this lane's image line (a column; a row when TR)
    const int ui = U0 - S3_LANE0 + (int)lane; // u coordinate of this lane's searched pixel (its window ends at uc)
    const uint32_t V0 = (TR ? 0u : p.row0) + tid.y * 4;
    const uint32_t vv = V0 + w;
    const uint32_t x = TR ? vv : (uint32_t)ui, y = TR ? (uint32_t)ui : vv;
    const int xi = (int)x;
    const bool is_out = lane >= (uint32_t)S3_LANE0 && x < p.w1 && y < p.row1;
    if (threadIdx.x == 0) {
        bb[0] = 0x7FFFFFFF;
        bb[1] = 0x7FFFFFFF;
        bb[2] = -0x7FFFFFFF;
        bb[3] = -0x7FFFFFFF;
        bb[4] = 0;
        bb[5] = 0;
        bb[6] = 0;
    }

    PixelSetup ps;
    ps.st1 = make_float2(0.0f, 1.0f);
    ps.e.cx = ps.e.cy = ps.e.ax = ps.e.ay = 0.0;
    ps.e.ox = ps.e.oy = 0;
    ps.r0 = ps.r1 = 0;
    // Lean plan, lanes along x, CorrParams::row_lines: a wave is one image row, and everything the setup below derives from
    // the epipolar line is the row's - it arrives as the row's table entry (RowLine; written by this pass's
    // search_range_kernel with row_line_of), wave-uniform, and no lane evaluates a line.  Per pixel: the interval, the
    // statistics word and the validity tests.
    constexpr bool ROWS = !STEP && !TR;
    const bool rows = ROWS && p.row_lines != 0;
    [[maybe_unused]] uint32_t row_m0 = 0u, row_flags = 0u; // (y is the wave's: scalar loads)
    [[maybe_unused]] bool row_mismatch = false; // (counting instantiations: a lane's own evaluation differs from the table)
    bool active;
    if (rows) {
        if (y < p.row1) {
            row_m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)row_table[y].m0);
            row_flags = (uint32_t)__builtin_amdgcn_readfirstlane((int)row_table[y].flags);
        }
        active = is_out && pixel_setup_row(p, x, y, stats1, range, (row_flags & RL_FINITE) != 0u, ps);
        if constexpr (COUNT && ROWS) {
            // every lane re-derives its row's entry from ITS pixel's line and interval: any difference poisons the candidate
            // count (as a missed bracket of the stepped walk does), so every test that compares counts checks the table
            if (x < p.w1 && y < p.row1) {
                const RowLine own = row_line_of(p, epipolar_line(p, x, y), active ? ps.r0 : (uint32_t)KERNEL_SIZE);
                const RowLine tab = row_table[y];
                row_mismatch = own.m0 != tab.m0 || own.flags != tab.flags || __double_as_longlong(own.ay) != __double_as_longlong(tab.ay);
            }
            if (counters && __any(row_mismatch) && lane == 0) atomicAdd(&counters[0], 1ull << 44);
        }
    } else {
        active = is_out && pixel_setup(p, x, y, stats1, range, ps);
    }
    const Line &e = ps.e;
    const uint32_t r0 = ps.r0, r1 = ps.r1;
    const int cs = p.corridor_size;
    const bool major_x = rows || e.ox == 0; // candidates advance along x (x2 == i exactly), stripes shift y

    // ---- this pixel's candidate set in displacement space ---------------------------------------------------
    // rectangle [lox, lox+wx) x [loy, loy+wy): every stripe keeps its minor coordinate over the interval; or, for
    // row-major lines that step inside the interval ("stepped"), the same rectangle with a row offset loy(dx)
    // that is re-evaluated per dx with the reference's own f64 expression (mod.rs:424-429).
    bool simple = true, stepped = false;
    // loose (stepped lanes only): at some candidates the reference's roundings move the upper stripes one row up - the line
    // passes within an ulp below a row 2^k, and v + off lands in the coarser binade exactly on the next integer - so that the
    // stripes occupy five of SIX consecutive rows.  Such a lane walks six planes per step, and where one of them passes the
    // filter the reference's own expression says which stripe - if any - it is (the hit branch).  The candidate counter
    // cannot afford that per plane: its instantiations leave such tiles to the candidate-by-candidate kernel, as before.
    bool loose = false;
    int lox = 0, loy = 0, lox_hi = 0, loy_hi = 0;
    uint32_t wx = 0, wy = 0;
    if (rows) {
        // the row's entry stands for the evaluation below: RL_SIMPLE is `constant && consecutive && m0 < 2^30 && cy == 0`
        // of this row's line (one m0 - the lean plan never looks at the far end), and what is left of `sane` is the pixel's
        // own interval (ilo <= r0 < 2^16 needs no test)
        if (active) {
            const uint32_t ilo = max(r0, (uint32_t)KERNEL_SIZE), ihi = min(r1, sat_sub_u32(p.w2, KERNEL_SIZE));
            simple = (row_flags & RL_SIMPLE) != 0u && (r1 - r0) <= CW_MAX_LEN;
            lox = (int)ilo - xi;
            lox_hi = lox;
            wx = ihi > ilo ? ihi - ilo : 0u;
            loy = (int)row_m0 - (int)y;
            loy_hi = loy;
            wy = (uint32_t)(2 * cs + 1);
        }
    } else if (active) {
        // (only the minor coordinate of candidate_xy is needed: the same operations on the selected coefficients)
        const double cmn = major_x ? e.cy : e.cx, amn = major_x ? e.ay : e.ax;
        const int omn = major_x ? e.oy : e.ox;
        const double vf = cmn * (double)r0 + amn, vl = STEP ? cmn * (double)(r1 - 1) + amn : vf;
        // (the lean plan: one floor where v - cs and v + cs share a binade, and never the far end - minor_rows)
        const MinorRows mr = minor_rows<STEP>(vf, vl, omn, cs);
        const uint32_t m0 = mr.m0, m0l = mr.m0l;
        const bool constant = mr.constant, consecutive = mr.consecutive, near = mr.near;
        const uint32_t lim2 = major_x ? p.w2 : p.h2;
        const uint32_t ilo = max(r0, (uint32_t)KERNEL_SIZE), ihi = min(r1, sat_sub_u32(lim2, KERNEL_SIZE));
        const uint32_t nmaj = ihi > ilo ? ihi - ilo : 0u;
        const bool sane = (r1 - r0) <= CW_MAX_LEN && m0 < 0x40000000u && m0l < 0x40000000u && ilo < 0x40000000u;
        simple = constant && consecutive && sane && (STEP || (major_x ? e.cy == 0.0 : e.cx == 0.0));
        // (m0, m0l >= 1: the casts of mod.rs:427-428 did not saturate a negative coordinate to 0)
        if (STEP && !simple && major_x != TR && (consecutive || (LOOSE_OK && near)) && sane && m0 >= 1u && m0l >= 1u && nmaj > 0u && nmaj <= 64u) {
            // the stripes must be consecutive rows at EVERY candidate, exactly as the reference rounds them:
            // floor((cy*i + ay) + off) == floor((cy*i + ay) - cs) + off + cs.  Where the fractional part is away
            // from 0 and 1 that is implied (the addition of a small integer is then exact enough); the few
            // positions where the line passes through an integer row are checked stripe by stripe.
            bool ok = consecutive, ok_near = true;
            // Every v = cy*i + ay of the interval lies between its two ends (the product and the sum round monotonically).
            // Where v - cs and v + cs share a binade for ALL of them - the two ends' extremes do, above 8 - every v + off
            // is exact (an integer added inside one binade), so the stripes are consecutive rows at every candidate without
            // looking at a single one: all pixels but those whose lines pass rows 16, 32, ... 2^k (+- the stripes).
            const double vlo = fmin(vf, vl) - (double)cs, vhi = fmax(vf, vl) + (double)cs;
            const bool one_binade = consecutive && vlo > 8.0 && vhi < 1.0e9 && (__double2hiint(vlo) >> 20) == (__double2hiint(vhi) >> 20);
            // (a running value screens the candidates: advanced by one addition per candidate it stays within 1e-10 of
            // the reference's own product-and-sum, so every position whose exact fractional part is outside
            // [2^-20, 1 - 2^-20] is among those it flags with 1e-6)
            const double cmin = TR ? e.cx : e.cy;
            double vs = cmin * (double)ilo + (TR ? e.ax : e.ay);
            for (uint32_t i = one_binade ? ihi : ilo; i < ihi; i++, vs += cmin) {
                const double fr = vs - floor(vs);
                if (!(fr >= 1.0e-6 && fr <= 1.0 - 1.0e-6)) {
                    // The reference's own value v = cy*i + ay (one product, one sum).  Where v - cs and v + cs lie in one
                    // binade and 8 < v < 1e9, every v + off (off = -cs .. cs, an integer) is exact, so floor(v + off) =
                    // floor(v - cs) + off + cs without looking: lines at exactly 45 degrees pass an integer row at EVERY
                    // candidate, and five candidate_xy per candidate made their setup 3x the walk.
                    {
                        const double v = cmin * (double)i + (TR ? e.ax : e.ay), lo = v - (double)cs, hi = v + (double)cs;
                        int elo, ehi;
                        (void)frexp(lo, &elo);
                        (void)frexp(hi, &ehi);
                        if (lo > 8.0 && elo == ehi && hi < 1.0e9) continue;
                    }
                    const CandXY c0 = candidate_xy(e, i, -cs);
                    const uint32_t b0 = TR ? c0.x : c0.y;
                    for (int off = -cs + 1; off <= cs; off++) {
                        const CandXY co = candidate_xy(e, i, off);
                        const uint32_t up = (TR ? co.x : co.y) - (b0 + (uint32_t)(off + cs));
                        ok = ok && up == 0u;
                        ok_near = ok_near && up <= 1u;
                    }
                }
            }
            loose = LOOSE_OK && !ok && ok_near;
            stepped = ok || loose;
        }
        if (major_x) {
            lox = (int)ilo - xi;
            lox_hi = lox;
            wx = nmaj;
            loy = (int)min(m0, m0l) - (int)y;
            loy_hi = (int)max(m0, m0l) - (int)y;
            wy = (uint32_t)(2 * cs + 1) + (loose ? 1u : 0u);
        } else {
            loy = (int)ilo - (int)y;
            loy_hi = loy;
            wy = nmaj;
            lox = (int)min(m0, m0l) - xi;
            lox_hi = (int)max(m0, m0l) - xi;
            wx = (uint32_t)(2 * cs + 1) + (loose ? 1u : 0u);
        }
    }
    const bool has = active && (simple || stepped) && wx > 0u && wy > 0u;
    // the same rectangle on the kernel's axes: [lou, lou+wu) along the lanes, [lov .. lov_hi, +wv) across the planes
    const int lou = TR ? loy : lox, lov = TR ? lox : loy, lov_hi = TR ? lox_hi : loy_hi;
    const uint32_t wu = TR ? wy : wx, wv = TR ? wx : wy;
    // wave-uniform bounds of the wave's displacement box
    const int mnx = wave_min_i32(has ? lou : 0x7FFFFFFF), mxx = wave_max_i32(has ? lou + (int)wu - 1 : -0x7FFFFFFF);
    // (across the planes - the lean plan's row of parallel lines: almost always the same two integers on every lane, one
    // comparison instead of two reductions)
    int mny = 0x7FFFFFFF, mxy = -0x7FFFFFFF;
    {
        const unsigned long long hm = __builtin_amdgcn_ballot_w64(has);
        const int fl = (int)__builtin_ctzll(hm | (1ull << 63));
        const int lo_f = __builtin_amdgcn_readlane(lov, fl), hi_f = __builtin_amdgcn_readlane(lov_hi + (int)wv - 1, fl);
        if (__builtin_amdgcn_ballot_w64(has && (lov != lo_f || lov_hi + (int)wv - 1 != hi_f))) {
            mny = wave_min_i32(has ? lov : 0x7FFFFFFF);
            mxy = wave_max_i32(has ? lov_hi + (int)wv - 1 : -0x7FFFFFFF);
        } else if (hm) {
            mny = lo_f;
            mxy = hi_f;
        }
    }
    const int need = wave_max_i32(has ? (int)min(wu * wv, 0x3FFFFFFFu) : 0);
    const bool wave_has = mxx >= mnx;
    const bool wave_odd = __any(active && !(simple || stepped));
    const bool wave_step = STEP && __any(has && stepped);
    const int wave_loose = STEP && LOOSE_OK && __any(has && loose) ? 1 : 0;
    // Lean plan: fold the two ends of the wave's union (DESIGN 4.2).  The wave walks n = mxx - mnx + 1 steps, the union of
    // its lanes' intervals [lo, hi]; where the intervals drift along the wave, the first steps are searched only at one end
    // of it and the last steps only at the other.  Low step k and high step n - K + k (k = 0 .. K-1) then run as ONE step,
    // every lane at the one of the two that its side of a seam takes - valid when each lane that searches one of them has its
    // 11 window columns (lanes l-10 .. l) on its own side: S12 = P(l) - P(l-11) only sums those.  Ascending (low steps at low
    // lanes): the pair breaks iff some lane a with lo_a <= k and some lane b <= a + 10 with hi_b >= n - K + k exist; with
    // Mh(a) = max hi over the lanes up to a + 10 lane a forbids exactly the K >= n + lo_a - Mh(a), so the largest K is the
    // wave's minimum of that, less one (and at most n / 2).  A lane takes the high step of pair k iff Mh(l) >= n - K + k: true
    // for a lane that searches it and for its ten lower neighbours, false for every lane up to one that searches step k.
    // Descending (low steps at high lanes): with ml(b) = min lo over the lanes up to b + 10, lane b forbids
    // K >= n + ml(b) - hi_b, and a lane takes the high step iff ml(l) > k.  One rule for the walk: fold_sel >= fold_base + k.
    [[maybe_unused]] int fold_k = 0, fold_base = 0, fold_sel = 0;
    [[maybe_unused]] bool fold_desc = false;
    if constexpr (!STEP) {
        if (p.box_fold && wave_has) {
            const int n = mxx - mnx + 1, lo = lou - mnx, hi = lo + (int)wu - 1;
            const int hpre = -wave_prefix_min_i32(has ? -hi : 1), lpre = wave_prefix_min_i32(has ? lo : 0x3FFFFFFF);
            const int up10 = (int)min(lane + 10u, 63u) * 4;
            const int mh = __builtin_amdgcn_ds_bpermute(up10, hpre), ml = __builtin_amdgcn_ds_bpermute(up10, lpre);
            const int ka = min(wave_min_i32(has ? n + lo - mh : 0x7FFFFFFF) - 1, n >> 1);
            const int kd = min(wave_min_i32(has ? n + ml - hi : 0x7FFFFFFF) - 1, n >> 1);
            fold_desc = kd > ka;
            fold_k = fold_desc ? kd : ka;
            fold_sel = fold_desc ? ml : mh;
            fold_base = fold_desc ? 1 : n - fold_k;
        }
    }
    // Stepped boxes: the wave's plane window at EVERY step, settled here, before the walk - lane t holds step t's.  A
    // lane's first plane at step t (displacement mnx + t) is floor(v(t)) - cs - v0 with v(t) the reference's own f64
    // evaluation of ITS line (mod.rs:424-429); in real arithmetic that line is g(t) = a + c t (a: its position relative to
    // the lane's own row at the wave's first step, c: its slope, |c| <= 1), and the f64 evaluation stays within 1e-11 of it.
    // The wave's lines are bracketed in fixed point, rounded outwards by more than that: a in [amin, amax] / 2^18,
    // c in [cmin, cmax] / 2^18, so at step t every searching lane's first plane lies in
    // [floor((amin + t cmin) / 2^18), floor((amax + t cmax) / 2^18)] - one plane wide unless the bracket straddles an
    // integer row there (affine F: the lanes' lines are parallel and - for a consistent pair - coincide, so that happens
    // where the line itself passes a row).  A window that is wider than needed only costs its planes: a lane re-derives its
    // OWN first plane, with the reference's expression, where a candidate of its passes the filter (the hit branch below).
    // The table has one step per lane, and the wide plan's boxes are up to ISP - 63 = 65 steps wide (eligibility below):
    // the one step past the lanes - step 64 - has its window in a wave-uniform word of its own (a lane number of 64
    // would wrap to lane 0, whose window on a sloped line holds other rows).
    constexpr int STEP_TABLE = 64;
    static_assert(ISP - 63 <= STEP_TABLE + 1, "a stepped wave walks at most the table's steps and step_last");
    int wave_planes = mxy - mny + 1; // never more than the wave's box is tall
    uint32_t step_tbl = 0u;          // lane t: {first plane of step t relative to mny | planes << 16}
    uint32_t step_last = 0u;         // the same for step 64 (wave-uniform)
    if (STEP && wave_step) {
        constexpr double FX = 262144.0; // 2^18
        double ga = 0.5, gc = 0.0;
        if (has) {
            ga = (double)(lov - mny) + 0.5;
            // (also for a lane whose stripes keep their rows over its own interval: its LINE is what the lanes beside it
            // follow - as a constant it would open the slope bracket to [0, c] and cost most steps a sixth plane)
            if (major_x != TR) {
                const double ii = (double)((TR ? (int)y : xi) + mnx);
                const double v2 = ((TR ? e.cx : e.cy) * ii + (TR ? e.ax : e.ay)) + (double)(-cs);
                ga = (v2 - (double)(TR ? xi : (int)y)) - (double)mny;
                gc = TR ? e.cx : e.cy;
            }
        }
        // (garbage in - a wave whose box the workgroup will decline - stays garbage, but inside int32)
        ga = fmin(fmax(ga, -4096.0), 4096.0);
        gc = fmin(fmax(gc, -2.0), 2.0);
        const int ai = (int)floor(ga * FX), ci = (int)floor(gc * FX);
        // (almost always every lane has the same two integers: one comparison instead of four reductions)
        const unsigned long long hm = __builtin_amdgcn_ballot_w64(has);
        const int fl = (int)__builtin_ctzll(hm | (1ull << 63));
        int amin = __builtin_amdgcn_readlane(ai, fl), amax = amin, cmin_i = __builtin_amdgcn_readlane(ci, fl), cmax_i = cmin_i;
        if (__builtin_amdgcn_ballot_w64(has && (ai != amin || ci != cmin_i))) {
            amin = wave_min_i32(has ? ai : 0x7FFFFFFF);
            amax = wave_max_i32(has ? ai : -0x7FFFFFFF);
            cmin_i = wave_min_i32(has ? ci : 0x7FFFFFFF);
            cmax_i = wave_max_i32(has ? ci : -0x7FFFFFFF);
        }
        const auto window = [&](int t) -> uint32_t { // (t >= 0: the products below keep their order)
            int lo = (amin - 1 + t * (cmin_i - 1)) >> 18, hi = (amax + 2 + t * (cmax_i + 2)) >> 18;
            // every lane's true first plane lies inside its own [lov, lov_hi] and so inside the wave's box
            lo = max(lo, 0);
            hi = max(min(hi, mxy - (2 * cs + 1 + wave_loose) + 1 - mny), lo);
            return (uint32_t)lo | ((uint32_t)(hi - lo + 2 * cs + 1 + wave_loose) << 16);
        };
        const int t = (int)lane;
        step_tbl = window(t);
        step_last = window(STEP_TABLE);
        wave_planes = min(wave_planes, max(wave_max_i32(t <= mxx - mnx ? (int)(step_tbl >> 16) : 0),
                                           mxx - mnx >= STEP_TABLE ? (int)(step_last >> 16) : 0));
    }
    __syncthreads(); // bb initialised
    if (lane == 0) {
        if (wave_has) {
            atomicMin(&bb[0], mnx);
            atomicMin(&bb[1], mny);
            atomicMax(&bb[2], mxx);
            atomicMax(&bb[3], mxy);
            atomicMax(&bb[4], need);
            atomicMax(&bb[6], wave_planes);
        }
        if (wave_odd) atomicOr(&bb[5], 1);
    }
    __syncthreads();
    const size_t pix = (size_t)y * p.w1 + x;
    const bool any_has = bb[2] >= bb[0];
    const int dx0 = bb[0], dy0 = bb[1];
    const int W = bb[2] - bb[0] + 1, H = bb[3] - bb[1] + 1;
    const int C0 = U0 - 6 + dx0; // target line (column; row when TR) of lane 0 at the box's first step
    const int C0a = TR ? C0 : (C0 & ~3);
    const int colshift = C0 - C0a;
    const int ncol = colshift + 64 + W - 1;
    bool eligible = !bb[5] && !(dbg & 4);
    if (any_has) {
        if (STEP) {
            // planes per step within what one 24-byte read serves at any alignment (14 - 3), the tall copy and the
            // statistics rows within the launch's LDS, and the walk (steps x planes per step) not much larger than
            // the largest pixel's own candidate set
            eligible = eligible && ncol <= LN && 64 + W - 1 <= ISP && bb[6] <= S3_MAXH && (uint32_t)(H + 26) <= 4u * PD &&
                       (uint32_t)(H + 3) <= p.box_sh && (long long)W * (bb[6] + 1) <= 3ll * bb[4] + 16;
        } else {
            eligible = eligible && ncol <= S3_COLS && H <= S3_MAXH && (long long)W * H <= 3ll * bb[4] + 16;
        }
    }
    if (!eligible || !any_has) {
        // nothing to search (every pixel None), or left to the candidate-by-candidate kernel
        if (is_out) {
            // contender words are only read for tiles on a work list: a declined tile hands its pixels over through
            // them; a tile with nothing to search is on no list and writes none
            const bool fb = active && !eligible;
            if (!eligible) contenders[pix] = fb ? (CW_FALLBACK << 60) : 0ull;
            if (!fb) out[pix] = CELL_NONE;
        }
        if (!eligible && threadIdx.x == 0) {
            if (counters && (dbg & 32)) { // diagnostics: declined workgroups, and why
                atomicAdd(&counters[3], 1ull);
                // one reason per run (bits 17:16 of the switch say which), counted above the candidates in counter 0
                int why = 3;
                if (bb[5]) why = 0;                                           // lines of different kinds in the tile
                else if (!(ncol <= LN && 64 + W - 1 <= ISP)) why = 1;          // displacement box too wide
                else if (STEP ? !(bb[6] <= S3_MAXH && (uint32_t)(H + 26) <= 4u * PD && (uint32_t)(H + 3) <= p.box_sh) : !(H <= S3_MAXH)) why = 2; // too tall
                if (why == ((dbg >> 16) & 3)) atomicAdd(&counters[0], 1ull << 36);
            }
            // a transposed tile is named by its first column and its index along y
            worklist_push(declined, TR ? (V0 | (tid.x << 16) | 0x40000000u) : ((uint32_t)U0 | (tid.y << 16)));
        }
        return;
    }
    if constexpr (COUNT && STEP) {
        // diagnostics (cvhip_ctx_get_box_counters; counters 4..7, apart from the four above): the stepped waves that
        // walk one step past the table's 64 lanes, and the most steps any stepped wave walks
        if (counters && lane == 0 && wave_step && wave_has) {
            const int nst = mxx - mnx + 1;
            if (nst == STEP_TABLE + 1) atomicAdd(&counters[TR ? 5 : 4], 1ull);
            atomicMax(&counters[6], (unsigned long long)nst);
        }
    }
    if constexpr (COUNT && !STEP) {
        // diagnostics (cvhip_ctx_get_box_fold_counters; counters 8..11): the steps of the waves' unions, the steps they walk
        // after folding, and the pairs folded in either orientation
        if (counters && lane == 0 && wave_has) {
            atomicAdd(&counters[8], (unsigned long long)(mxx - mnx + 1));
            atomicAdd(&counters[9], (unsigned long long)(mxx - mnx + 1 - fold_k));
            if (fold_k) atomicAdd(&counters[fold_desc ? 11 : 10], (unsigned long long)fold_k);
        }
    }
    const int NPL = H > 9 ? S3_MAXH : (H > 5 ? 9 : 5); // planes staged (lean: group A = 0..4, group B = 5..8)
    if (dbg & 256) return; // profiling: per-pixel setup and box reduction only

    // ---- stage the target lines (lean: 4 row-shifted copies of 20 bytes; stepped: one tall copy) and the candidate
    // statistics ---------------------------------------------------------------------------------------------
    if (!(dbg & 512)) {
        const int R0 = (int)V0 + dy0 - KERNEL_SIZE; // first v coordinate of copy 0 / of the tall copy
        if constexpr (STEP) {
            // bytes R0 .. R0 + 4*nk - 1 of every line: whatever offset w + s0 <= H + 2 a wave reads its 24 bytes at
            const int nk = (H + 26 + 3) >> 2; // <= PD (eligibility)
            uint32_t *const cols = reinterpret_cast<uint32_t *>(lds);
            if (!TR) {
                // lines are columns: the bytes along v are a column of the image, gathered by 4x4 byte transposes
                const int nb = (ncol + 3) >> 2;
                // (inside the image: no bounds tests, no division, byte permutes - see the lean plan below)
                const bool inside = R0 >= 0 && R0 + 4 * nk <= (int)p.h2 && C0a >= 0 && C0a + 4 * nb <= (int)p.w2;
                if (inside && nb <= 32) {
                    const int b = (int)(threadIdx.x & 31u);
                    if (b < nb) {
                        const uint8_t *const col_base = img2 + (size_t)R0 * p.w2 + (size_t)(C0a + 4 * b);
                        uint32_t *const dst0 = cols + (uint32_t)(4 * b) * PD;
                        for (int k = (int)(threadIdx.x >> 5); k < nk; k += 8) {
                            const uint8_t *src = col_base + (size_t)(4 * k) * p.w2;
                            uint32_t d0, d1, d2, d3;
                            __builtin_memcpy(&d0, src, 4);
                            __builtin_memcpy(&d1, src + p.w2, 4);
                            __builtin_memcpy(&d2, src + 2 * (size_t)p.w2, 4);
                            __builtin_memcpy(&d3, src + 3 * (size_t)p.w2, 4);
                            const uint32_t p01 = __builtin_amdgcn_perm(d1, d0, 0x05010400u), q01 = __builtin_amdgcn_perm(d1, d0, 0x07030602u);
                            const uint32_t p23 = __builtin_amdgcn_perm(d3, d2, 0x05010400u), q23 = __builtin_amdgcn_perm(d3, d2, 0x07030602u);
                            uint32_t *dst = dst0 + k;
                            dst[0] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
                            dst[PD] = __builtin_amdgcn_perm(p23, p01, 0x07060302u);
                            dst[2 * PD] = __builtin_amdgcn_perm(q23, q01, 0x05040100u);
                            dst[3 * PD] = __builtin_amdgcn_perm(q23, q01, 0x07060302u);
                        }
                    }
                } else
                for (int u = (int)threadIdx.x; u < nk * nb; u += 256) {
                    const int k = u / nb, b = u - k * nb;
                    const int rr = R0 + 4 * k, col = C0a + 4 * b;
                    const uint32_t d0 = load_dword_checked(img2, (int)p.w2, (int)p.h2, rr + 0, col);
                    const uint32_t d1 = load_dword_checked(img2, (int)p.w2, (int)p.h2, rr + 1, col);
                    const uint32_t d2 = load_dword_checked(img2, (int)p.w2, (int)p.h2, rr + 2, col);
                    const uint32_t d3 = load_dword_checked(img2, (int)p.w2, (int)p.h2, rr + 3, col);
                    uint32_t *dst = cols + (uint32_t)(4 * b) * PD + (uint32_t)k; // (4 * b + 3 < LN: ncol <= LN, LN a multiple of 4)
                    dst[0] = (d0 & 0xFFu) | ((d1 & 0xFFu) << 8) | ((d2 & 0xFFu) << 16) | (d3 << 24);
                    dst[PD] = ((d0 >> 8) & 0xFFu) | (d1 & 0xFF00u) | ((d2 & 0xFF00u) << 8) | ((d3 & 0xFF00u) << 16);
                    dst[2 * PD] = ((d0 >> 16) & 0xFFu) | ((d1 >> 8) & 0xFF00u) | (d2 & 0xFF0000u) | ((d3 & 0xFF0000u) << 8);
                    dst[3 * PD] = (d0 >> 24) | ((d1 >> 16) & 0xFF00u) | ((d2 >> 8) & 0xFF0000u) | (d3 & 0xFF000000u);
                }
            } else {
                // lines are rows: the bytes along v are contiguous in the image
                const bool inside = C0a >= 0 && C0a + ncol <= (int)p.h2 && R0 >= 0 && R0 + 4 * nk <= (int)p.w2;
                if (inside && ncol <= 128) { // (no bounds tests, no division: a thread keeps its line and walks the dwords)
                    const int c = (int)(threadIdx.x & 127u);
                    if (c < ncol) {
                        const uint8_t *src = img2 + (size_t)(C0a + c) * p.w2 + (size_t)R0;
                        uint32_t *const dst = cols + (uint32_t)c * PD;
                        for (int k = (int)(threadIdx.x >> 7); k < nk; k += 2) {
                            uint32_t d;
                            __builtin_memcpy(&d, src + 4 * k, 4);
                            dst[k] = d;
                        }
                    }
                } else
                for (int u = (int)threadIdx.x; u < nk * ncol; u += 256) {
                    const int k = u / ncol, c = u - k * ncol;
                    cols[(uint32_t)c * PD + (uint32_t)k] = load_dword_checked(img2, (int)p.w2, (int)p.h2, C0a + c, R0 + 4 * k);
                }
            }
        } else if (!TR) {
            // lines are columns: the bytes along v are a column of the image, gathered by 4x4 byte transposes
            const int nb = (ncol + 3) >> 2;
            const int units = 4 * NDW * nb;
            // Almost every workgroup's staged block lies inside the image: then the loads need no bounds tests, the unit
            // index no division (a thread keeps its column group b and walks the 4 x NDW (copy, dword) pairs), and the
            // transposes are byte permutes.  Five planes never read the tail dword (planes 0..4 end at byte 14).
            const bool inside = R0 >= 0 && R0 + 3 + 4 * (NDW - 1) + 3 < (int)p.h2 && C0a >= 0 && C0a + 4 * nb <= (int)p.w2;
            if (inside && nb <= 32) {
                const int b = (int)(threadIdx.x & 31u);
                const int kmax = NPL > 5 ? NDW : NDW - 1;
                if (b < nb) {
                    const uint8_t *const col_base = img2 + (size_t)R0 * p.w2 + (size_t)(C0a + 4 * b);
                    for (int wk = (int)(threadIdx.x >> 5); wk < 4 * NDW; wk += 8) {
                        const int cw = wk / NDW, k = wk - cw * NDW;
                        if (k >= kmax) continue;
                        const uint8_t *src = col_base + (size_t)(cw + 4 * k) * p.w2;
                        uint32_t d0, d1, d2, d3;
                        __builtin_memcpy(&d0, src, 4);
                        __builtin_memcpy(&d1, src + p.w2, 4);
                        __builtin_memcpy(&d2, src + 2 * (size_t)p.w2, 4);
                        __builtin_memcpy(&d3, src + 3 * (size_t)p.w2, 4);
                        // v_perm_b32: selector bytes 0-3 pick from the second operand, 4-7 from the first
                        const uint32_t p01 = __builtin_amdgcn_perm(d1, d0, 0x05010400u), q01 = __builtin_amdgcn_perm(d1, d0, 0x07030602u);
                        const uint32_t p23 = __builtin_amdgcn_perm(d3, d2, 0x05010400u), q23 = __builtin_amdgcn_perm(d3, d2, 0x07030602u);
                        uint4 t; // t.c = rows rr..rr+3 of column col + c
                        t.x = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
                        t.y = __builtin_amdgcn_perm(p23, p01, 0x07060302u);
                        t.z = __builtin_amdgcn_perm(q23, q01, 0x05040100u);
                        t.w = __builtin_amdgcn_perm(q23, q01, 0x07060302u);
                        if (k < 4) {
                            uint32_t *dst = reinterpret_cast<uint32_t *>(lds + S3_B16_OFF + (size_t)(cw * S3_COLS + 4 * b) * 16u) + k;
                            dst[0] = t.x;
                            dst[4] = t.y;
                            dst[8] = t.z;
                            dst[12] = t.w;
                        } else {
                            *reinterpret_cast<uint4 *>(lds + S3_TAIL_OFF + (size_t)(cw * S3_COLS + 4 * b) * 4u) = t;
                        }
                    }
                }
            } else
            for (int u = (int)threadIdx.x; u < units; u += 256) {
                const int wk = u / nb, b = u - wk * nb; // wk = copy * NDW + k
                const int cw = wk / NDW, k = wk - cw * NDW;
                const int rr = R0 + cw + 4 * k, col = C0a + 4 * b;
                const uint32_t d0 = load_dword_checked(img2, (int)p.w2, (int)p.h2, rr + 0, col);
                const uint32_t d1 = load_dword_checked(img2, (int)p.w2, (int)p.h2, rr + 1, col);
                const uint32_t d2 = load_dword_checked(img2, (int)p.w2, (int)p.h2, rr + 2, col);
                const uint32_t d3 = load_dword_checked(img2, (int)p.w2, (int)p.h2, rr + 3, col);
                uint4 t; // 4x4 byte transpose: t.c = rows rr..rr+3 of column col + c
                t.x = (d0 & 0xFFu) | ((d1 & 0xFFu) << 8) | ((d2 & 0xFFu) << 16) | (d3 << 24);
                t.y = ((d0 >> 8) & 0xFFu) | (d1 & 0xFF00u) | ((d2 & 0xFF00u) << 8) | ((d3 & 0xFF00u) << 16);
                t.z = ((d0 >> 16) & 0xFFu) | ((d1 >> 8) & 0xFF00u) | (d2 & 0xFF0000u) | ((d3 & 0xFF0000u) << 8);
                t.w = (d0 >> 24) | ((d1 >> 16) & 0xFF00u) | ((d2 >> 8) & 0xFF0000u) | (d3 & 0xFF000000u);
                if (k < 4) {
                    uint32_t *dst = reinterpret_cast<uint32_t *>(lds + S3_B16_OFF + (size_t)(cw * S3_COLS + 4 * b) * 16u) + k;
                    dst[0] = t.x;
                    dst[4] = t.y;
                    dst[8] = t.z;
                    dst[12] = t.w;
                } else {
                    *reinterpret_cast<uint4 *>(lds + S3_TAIL_OFF + (size_t)(cw * S3_COLS + 4 * b) * 4u) = t;
                }
            }
        } else {
            // lines are rows: the bytes along v are contiguous in the image
            const int units = 4 * NDW * ncol;
            const bool inside = C0a >= 0 && C0a + ncol <= (int)p.h2 && R0 >= 0 && R0 + 3 + 4 * NDW <= (int)p.w2;
            if (inside && ncol <= 128) { // (as above; five planes never read the tail dword)
                const int c = (int)(threadIdx.x & 127u);
                const int kmax = NPL > 5 ? NDW : NDW - 1;
                if (c < ncol) {
                    const uint8_t *src = img2 + (size_t)(C0a + c) * p.w2 + (size_t)R0;
                    for (int wk = (int)(threadIdx.x >> 7); wk < 4 * NDW; wk += 2) {
                        const int cw = wk / NDW, k = wk - cw * NDW;
                        if (k >= kmax) continue;
                        uint32_t d;
                        __builtin_memcpy(&d, src + cw + 4 * k, 4);
                        if (k < 4)
                            *(reinterpret_cast<uint32_t *>(lds + S3_B16_OFF + (size_t)(cw * S3_COLS + c) * 16u) + k) = d;
                        else
                            *(reinterpret_cast<uint32_t *>(lds + S3_TAIL_OFF + (size_t)(cw * S3_COLS + c) * TAIL_BYTES) + (k - 4)) = d;
                    }
                }
            } else
            for (int u = (int)threadIdx.x; u < units; u += 256) {
                const int wk = u / ncol, c = u - wk * ncol; // wk = copy * NDW + k
                const int cw = wk / NDW, k = wk - cw * NDW;
                const uint32_t d = load_dword_checked(img2, (int)p.w2, (int)p.h2, C0a + c, R0 + cw + 4 * k);
                if (k < 4)
                    *(reinterpret_cast<uint32_t *>(lds + S3_B16_OFF + (size_t)(cw * S3_COLS + c) * 16u) + k) = d;
                else
                    *(reinterpret_cast<uint32_t *>(lds + S3_TAIL_OFF + (size_t)(cw * S3_COLS + c) * TAIL_BYTES) + (k - 4)) = d;
            }
        }
        const int isp = 64 + W - 1, isrows = (STEP ? H : NPL) + 3;
        const int gu0 = U0 - S3_LANE0 + dx0; // target u of lane 0's pixel at the box's first step
        const int gv0 = (int)V0 + dy0;
        const bool is_inside = gv0 >= 0 && gu0 >= 0 && gv0 + isrows <= (int)(TR ? p.w2 : p.h2) && gu0 + isp <= (int)(TR ? p.h2 : p.w2);
        if (is_inside && isp <= 128) { // (as above: a thread keeps its cell column and walks the rows two at a time)
            const int c = (int)(threadIdx.x & 127u);
            if (c < isp) {
                const uint2 *src = istats2 + (TR ? (size_t)(gu0 + c) * p.w2 + (size_t)gv0 : (size_t)gv0 * p.w2 + (size_t)(gu0 + c));
                const size_t pitch = TR ? (size_t)1 : (size_t)p.w2;
                for (int r = (int)(threadIdx.x >> 7); r < isrows; r += 2) {
                    const uint2 tt = src[(size_t)r * pitch];
                    const bool ok = (tt.x & 0x80000000u) != 0u;
                    *reinterpret_cast<uint2 *>(lds + S3_IS_OFF + (size_t)(r * ISP + c) * 8u) =
                        make_uint2(ok ? 0u - (tt.x & 0x7FFFFFFFu) : 0u, ok ? (RS ? __float_as_uint(__builtin_amdgcn_rcpf(__uint_as_float(tt.y))) : tt.y) : NO_CAND);
                }
            }
        } else
        for (int u = (int)threadIdx.x; u < isp * isrows; u += 256) {
            const int r = u / isp, c = u - r * isp;
            const int gv = (int)V0 + dy0 + r, gu = gu0 + c;
            const int gx = TR ? gv : gu, gy = TR ? gu : gv;
            // {-window sum, f32 stdev - the lean plan: its reciprocal (v_rcp_f32: within an ulp, part of the approximate score, see record())};
            // centres outside the image or skipped by the reference (stdev non-finite or < min_stdev, mod.rs:430-441) get +inf - the
            // lean plan: 0 - and never pass the pre-screen
            uint2 v = make_uint2(0u, NO_CAND);
            if (gy >= 0 && gy < (int)p.h2 && gx >= 0 && gx < (int)p.w2) {
                const uint2 tt = istats2[(size_t)gy * p.w2 + (size_t)gx];
                if (tt.x & 0x80000000u) // -s2: N = 121*S12 + s1*(-s2) is one mul + one mad
                    v = make_uint2(0u - (tt.x & 0x7FFFFFFFu), RS ? __float_as_uint(__builtin_amdgcn_rcpf(__uint_as_float(tt.y))) : tt.y);
            }
            *reinterpret_cast<uint2 *>(lds + S3_IS_OFF + (size_t)(r * ISP + c) * 8u) = v;
        }
    }
    // this lane's searched line (column uc, or row uc when TR), v-5 .. v+5, packed and pre-shifted by 0..3 bytes
    uint32_t a[4][4];
    {
        uint32_t a0 = 0, a1 = 0, a2 = 0;
        if (!TR && uc >= 0 && uc < (int)p.w1 && vv >= (uint32_t)KERNEL_SIZE && vv + KERNEL_SIZE < p.h1) {
            const uint8_t *pc = img1 + (size_t)(vv - KERNEL_SIZE) * p.w1 + (size_t)uc;
            uint32_t b[KERNEL_WIDTH];
#pragma unroll
            for (int r = 0; r < KERNEL_WIDTH; r++) b[r] = pc[(size_t)r * p.w1];
            a0 = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            a1 = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            a2 = b[8] | (b[9] << 8) | (b[10] << 16);
        }
        if (TR && uc >= 0 && uc < (int)p.h1 && vv >= (uint32_t)KERNEL_SIZE && vv + KERNEL_SIZE < p.w1) {
            const Row12 rr = load_row12(img1 + (size_t)uc * p.w1 + (vv - KERNEL_SIZE));
            a0 = rr.a;
            a1 = rr.b;
            a2 = rr.c & 0x00FFFFFFu;
        }
        a[0][0] = a0;
        a[0][1] = a1;
        a[0][2] = a2;
        a[0][3] = 0u;
#pragma unroll
        for (int q = 1; q < 4; q++) { // 128-bit left shift by q bytes
            a[q][0] = a0 << (8 * q);
            a[q][1] = __builtin_amdgcn_alignbyte(a1, a0, 4 - q);
            a[q][2] = __builtin_amdgcn_alignbyte(a2, a1, 4 - q);
            a[q][3] = __builtin_amdgcn_alignbyte(0u, a2, 4 - q);
        }
    }
    const uint32_t s1 = has ? (istats1[pix].x & 0x7FFFFFFFu) : 0u;
    const float k1 = ps.st1.y * (float)(KERNEL_POINT_COUNT * KERNEL_POINT_COUNT); // 121*121*sd1
    __syncthreads();

    unsigned long long word = 0ull;
    uint2 cell = make_uint2(CELL_NONE, 0x7FC00000u);
    uint32_t evaluated = 0, whole = 0, exact_evals = 0;
    const float thr_lo = p.threshold - S2_DELTA;
    // Contender bookkeeping, in the pre-screen's own domain.  A candidate's x = (float)N * r - the exact product, r = the
    // rounded 1 / sd2 (lean plan: the staged table's; stepped plan: v_rcp_f32 of the staged stdev) - stands for its approximate
    // score g = x / k1; g has fewer roundings than the chain's own f32 steps allow for, so |f - g| <= DELTA holds for it.  The
    // state is one number per lane, T = max(T0, fl(R + D)), R the largest x recorded so far:
    //     D  = k1 * (2 DELTA + 2^-20)   the band, widened by 2^-20 (16 ulp of a score) for the roundings below
    //     T0 = fl(lam + 2 D),  lam = thr_lo * k1 shaved by 2^-18 of itself and 2^-20 D
    // Pre-screen (walk and hit branch): fl(x - T) >= -2 D - one fma against the state, no bound to rebuild.
    // Restart (the list starts anew with this candidate): fl(x - T) > 0, i.e. x > T exactly.
    // Record: T = max(T, fl(x + D)) - one fma and one v_max_f32; the lean plan's code is a scalar (plane << 7 | step) that the
    // lane turns into the reference's (stripe << 11 | i - r0) after the walk, the stepped plans' codes are built per lane.
    // The invariant the exact phase needs: every candidate with g >= max(G - 2 DELTA, thr_lo), G = R_final / k1, reaches it
    // (is on the final list, or the list overflowed).  The roundings that enter, with |x|, |R| < 1.01 k1 (|g| <= 1 + DELTA):
    // fl(R + D), fl(T - 2 D), the stepped plans' fl(limk sd2) and the fmas each within 1.02 k1 2^-24 (the reciprocal's error is
    // inside x, hence inside g), D itself within D 2^-24 - together below 8 k1 2^-24 of the 2^-20 k1 in D.  So (a) a candidate
    // that fails the pre-screen has x < T - 2 D + 3 k1 2^-24: below R - 2 DELTA k1 where T = fl(R + D), below thr_lo k1 where
    // T = T0 (the shaves of lam exceed T0's rounding at any threshold); (b) a restart has x_new > fl(R + D) >= R + D -
    // 1.02 k1 2^-24, so everything it drops lies below x_new - 2 DELTA k1 <= R_final - 2 DELTA k1.  The few candidates the
    // widening lets through only join the list.  (A pixel's first record at x <= T0 - rare: g within 2 DELTA of thr_lo - starts
    // the list through the append path.)  For thr_lo > 1e-10 lam > 2^-23 D, so T0 > 2 D and the lean plan's cells without a
    // candidate (r = 0: x = 0) never pass, as before.  Lanes without candidates have T = +inf.
    const float D = k1 * (2.0f * S2_DELTA + 9.5367431640625e-7f), M = -2.0f * D;
    const auto start_of = [&]() -> float {
        float lam = thr_lo * k1;
        lam -= fabsf(lam) * 3.814697265625e-6f + D * 9.5367431640625e-7f;
        return lam + 2.0f * D;
    };
    float T = has ? start_of() : __builtin_inff();
    float limk = T + M; // (stepped plans: the walk's bound on (float)N / sd2, kept beside T)
    // bits 15 j: the codes, oldest first; bits 60..63: how many were recorded (S2_K + 1: more than the list holds)
    unsigned long long clist = 0ull;
    const auto max_f32 = [](float a, float b) -> float { // v_max_f32 as it is: no operand is ever a NaN here, and fmaxf()
        float r;                                          // spends an instruction per operand on quieting signalling ones
        asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
        return r;
    };
    auto record = [&](bool restart, float t, uint32_t code) { // t = fl(x + D)
        // Nearly every record is a restart, so it is a path of its own (one 64-bit move); appending inside the band - the
        // variable 64-bit shift, the count's cap - is a real branch that almost no wave takes.
        if (restart) {
            clist = (1ull << 60) | code;
        } else {
            uint32_t count = (uint32_t)(clist >> 60);
            asm volatile("" : "+v"(count)); // (keeps the two paths apart: as selects the append costs every record its dozen operations)
            if (count < (uint32_t)S2_K) clist |= (unsigned long long)code << (15u * count);
            clist = (clist & ((1ull << 60) - 1ull)) | ((unsigned long long)min(count + 1u, (uint32_t)S2_K + 1u) << 60);
        }
        T = max_f32(T, t);
        if (STEP) limk = T + M;
    };

    // mod.rs:424-429 for stripe -cs at displacement dx, the reference's own operations: this lane's first plane at that step.
    // The value lies between the stripe's rows at the two ends of the pixel's interval (both >= 1 and < 2^30: setup), so the
    // saturating cast of the reference is a plain one here.
    const auto step_first_plane = [&](int dx) -> int {
        const double ii = (double)((TR ? (int)y : xi) + dx);
        const double v2 = ((TR ? e.cx : e.cy) * ii + (TR ? e.ax : e.ay)) + (double)(-cs);
        return (int)floor(v2) - (TR ? xi : (int)y);
    };
    [[maybe_unused]] bool bracket_missed = false;
    if (wave_has && !(dbg & 8)) {
        const uint32_t col0 = lane + (uint32_t)colshift + (uint32_t)(mnx - dx0);
        const uint8_t *const bB16 = lds + S3_B16_OFF + (w * S3_COLS + col0) * 16u;
        const uint8_t *const bB4 = lds + S3_TAIL_OFF + (w * S3_COLS + col0) * (uint32_t)TAIL_BYTES;
        const uint32_t *const bCOL = reinterpret_cast<const uint32_t *>(lds) + col0 * PD; // (stepped: the tall copy)
        const uint8_t *const bIS = lds + S3_IS_OFF + (w * ISP + lane + (uint32_t)(mnx - dx0)) * 8u;
        const int idx_lo = (int)(lane >= 11u ? lane - 11u : 0u) * 4;
        const int nsteps = mxx - mnx + 1;
        const int ws0 = mny - dy0, wn = mxy - mny + 1; // the wave's plane window while no line steps
        [[maybe_unused]] const int WV = 2 * cs + 1; // planes of one pixel at one step (its stripes)
        // Inside out: from the middle of the wave's displacement range up to its end, then from the middle down to
        // its start.  The ranges are centred on the positions predicted by the previous level, so the best matches
        // sit around the middle and are met first; the near-misses next to them (which pass the initial threshold
        // and would each cost a trip through the hit branch) then come after the bound has risen.  Any order is exact.
        // Lean plan: that is the order of the steps [K, n - K) nobody folded; the K folded pairs - the ends of the range - come
        // after them, pair K-1 first, and there `step` is the lane's own: the low or the high step of the pair (setup).  The
        // step's body is the BOX_STEP_SECTION at the top of this file, included once per loop.
        const int nmid = nsteps - 2 * fold_k, nwalk = nsteps - fold_k;
        const int mid = nmid >> 1;
#define BOX_STEP_SECTION
        if constexpr (STEP) {
            for (int t = 0; t < nsteps; t++) {
                const int step = t < nsteps - mid ? mid + t : nsteps - 1 - t;
#include "box_body.inc"
            }
        } else {
            for (int t = 0; t < nmid; t++) {
                const int step = fold_k + (t < nmid - mid ? mid + t : nmid - 1 - t);
#include "box_body.inc"
            }
            for (int k = fold_k - 1; k >= 0; k--) {
                const int step = fold_sel >= fold_base + k ? nwalk + k : k;
#include "box_body.inc"
            }
        }
#undef BOX_STEP_SECTION
    }

    // ---- exact re-evaluation of the contenders: mod.rs:442-464, the reference's serial f32 chain and acceptance rule; the
    // list is unordered here, so "first maximum" is the smallest code among equals.
    // How many evaluations this lane's pixel needs: none if it has no contender, if it re-evaluates its whole corridor
    // elsewhere, or - a pass whose scores nobody can read (CorrParams::need_scores) - if ONE contender is in the band: every
    // other candidate then has g < g* - 2 delta, i.e. f < f*, and g* >= threshold + delta means f* >= threshold; the match
    // is that contender, the 121-term chain could only add the score, and the cell keeps g*.
    const uint32_t count = (uint32_t)(clist >> 60);
    clist &= (1ull << 60) - 1ull;
    if (!STEP) {
        // the lean walk recorded (plane << 7 | step): the candidate at displacement (mnx + step, dy0 + plane) on the kernel's
        // axes; its code (stripe << 11 | i - r0) on the image's, with the position along the lanes where the line runs along them
        const bool pu = major_x != TR;
        unsigned long long codes = 0ull;
        for (uint32_t j = 0; j < min(count, (uint32_t)S2_K); j++) {
            const uint32_t rel = (uint32_t)(clist >> (15u * j)) & 0x7FFFu;
            const int du = mnx + (int)(rel & 127u), dv = dy0 + (int)(rel >> 7);
            const uint32_t code = pu ? ((uint32_t)(dv - lov) << 11) | (uint32_t)(ui + du - (int)r0)
                                     : ((uint32_t)(du - lou) << 11) | (uint32_t)((int)vv + dv - (int)r0);
            codes |= (unsigned long long)code << (15u * j);
        }
        clist = codes;
    }
    uint32_t ecount = 0;
    Line ex = e;
    // The candidate (x | y << 16) that a contender code (stripe << 11 | i - r0) names: candidate_xy of the pixel's line.  With
    // the row table no line is evaluated: the lane is `simple` on a row-major line with cx = 1, ax = 0, cy = +-0 - so
    // x2 = floor(1.0 * i + 0.0) = i, and y2 = floor((+-0 * i + ay) + off) is the row of stripe off + cs at ANY i, which setup
    // found `constant` and `consecutive` from m0 for exactly this: y2 = m0 + stripe.  Both as integers.
    const auto cand_of = [&](uint32_t code) -> uint32_t {
        if (rows) {
            const uint32_t cxy = (r0 + (code & 0x7FFu)) | ((row_m0 + (code >> 11)) << 16);
            if constexpr (COUNT && ROWS) { // (the counting instantiations evaluate the line all the same, and compare)
                const CandXY c = candidate_xy(epipolar_line(p, x, y), r0 + (code & 0x7FFu), (int)(code >> 11) - cs);
                if (cxy != (c.x | (c.y << 16))) row_mismatch = true;
            }
            return cxy;
        }
        const CandXY c = candidate_xy(ex, r0 + (code & 0x7FFu), (int)(code >> 11) - cs);
        return c.x | (c.y << 16);
    };
    if (has) {
        if (count > (uint32_t)S2_K) {
            word = CW_WHOLE << 60;
            whole = 1;
            evaluated = 0; // the exact kernel walks (and counts) the whole corridor
        } else if (count > 0u && !(dbg & (16 | 512))) { // (512: the contenders come from unstaged LDS)
            // Rectified instantiation: the epipolar line is not needed during the walk, so it is re-derived here (same
            // expressions, same bits) instead of living in 8 registers across it.
            if (!STEP && !rows) {
                uint32_t xo = x, yo = y;
                asm volatile("" : "+v"(xo), "+v"(yo));
                ex = epipolar_line(p, xo, yo);
            }
            ecount = count;
            // (the one contender is the last record and a restart or the only one: T = fl(x* + D) where T > T0, and then
            // g* = x* / k1 >= threshold + DELTA follows from the test below with 2^-18 to spare for its roundings; the score
            // the cell keeps is that g* to within them - a pass without scores never writes it)
            const float T0 = start_of();
            if (!p.need_scores && count == 1u && T > T0 && T - D >= (p.threshold + S2_DELTA + 3.814697265625e-6f) * k1) {
                cell = make_uint2(cand_of((uint32_t)clist & 0x7FFFu), __float_as_uint((T - D) * __builtin_amdgcn_rcpf(k1)));
                ecount = 0u;
            }
        }
    }
    // one evaluation: pixel (px, py) of image 1 against the candidate at (qx, qy) of image 2 - everything re-derived from
    // the coordinates (window statistics included: the same loads, the same bits), so that ANY lane can run it
    const auto chain = [&](uint32_t px, uint32_t py, uint32_t qx, uint32_t qy) -> float {
        const float2 st1x = stats_of(stats1[(size_t)py * p.w1 + px]);
        const uint2 is2 = istats2[(size_t)qy * p.w2 + qx];
        const float avg1 = st1x.x, sdev1 = st1x.y;
        const float avg2 = (float)(is2.x & 0x7FFFFFFFu) / (float)KERNEL_POINT_COUNT; // == compute_point_avg
        const float sdev2 = __uint_as_float(is2.y);
        const uint8_t *base1 = img1 + (size_t)(py - KERNEL_SIZE) * p.w1 + (px - KERNEL_SIZE);
        const uint8_t *base2 = img2 + (size_t)(qy - KERNEL_SIZE) * p.w2 + (qx - KERNEL_SIZE);
        float corr = 0.0f;
        // Both windows come straight from L1/L2 (one contender per pixel is the rule, so nothing is re-read), in three
        // batches of rows (a real loop): all 22 row loads in flight at once would make this phase the kernel's register
        // high-water mark (83 instead of ~50) and cost the walk its occupancy.
#pragma unroll 1
        for (int rb = 0; rb < 12; rb += 4) {
            Row12 av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int rr = min(rb + r, KERNEL_WIDTH - 1);
                av[r] = load_row12(base1 + (size_t)rr * p.w1);
                bv[r] = load_row12(base2 + (size_t)rr * p.w2);
            }
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (rb + r < KERNEL_WIDTH) corr = row_corr_acc(corr, av[r], bv[r], avg1, avg2);
        }
        return corr / (sdev1 * sdev2 * (float)KERNEL_POINT_COUNT); // mod.rs:454
    };
    bool have = false;
    float bcorr = 0.0f;
    uint32_t bxy = 0, bcode = 0;
    const auto consider = [&](float corr, uint32_t code, uint32_t cxy) { // mod.rs:456-464
        if (corr >= p.threshold && (!have || corr > bcorr || (corr == bcorr && code < bcode))) {
            have = true;
            bcorr = corr;
            bcode = code;
            bxy = cxy;
        }
    };
    // A second and third contender are rare per pixel (a few per cent) but not per wave: with each lane working through its
    // own list nearly every wave paid two or three passes of the 550-instruction chain for a handful of lanes.  The lanes
    // with nothing to evaluate - the 11 halo lanes, pixels without a match, single contenders of a scoreless pass - take
    // them instead: every lane keeps its first contender, the others go through a small queue in LDS (the wave's own copy
    // of the target lines - dead after the walk; the stepped plans share one tall copy, hence their barrier) and the
    // results come back the same way.  The chain, its operands and the selection rule are unchanged.
    constexpr uint32_t QCAP = 128;
    if constexpr (STEP) __syncthreads(); // (every wave is through with the staged lines)
    uint32_t *const q_pix = reinterpret_cast<uint32_t *>(STEP ? lds + w * (QCAP * 12u) : lds + S3_B16_OFF + w * (S3_COLS * 16u));
    uint32_t *const q_cand = q_pix + QCAP;
    float *const q_corr = reinterpret_cast<float *>(q_cand + QCAP);
    static_assert(QCAP * 12u <= S3_COLS * 16u, "the queue lives in one wave's copy of the target lines");
    uint32_t extras = ecount > 1u ? ecount - 1u : 0u;
    uint32_t q_incl = wave_prefix_sum(extras);
    uint32_t q_total = (uint32_t)__builtin_amdgcn_readlane((int)q_incl, 63);
    if (q_total > QCAP) {
        // more second contenders than the queue holds (never seen outside synthetic ties): the pixels behind the limit
        // re-evaluate their whole corridor in the fallback kernel instead - the same search, done the long way
        if (q_incl > QCAP && extras > 0u) {
            word = CW_WHOLE << 60;
            whole = 1;
            evaluated = 0;
            ecount = 0;
            extras = 0;
        }
        q_incl = wave_prefix_sum(extras);
        q_total = (uint32_t)__builtin_amdgcn_readlane((int)q_incl, 63);
    }
    const uint32_t q_base = q_incl - extras;
    for (uint32_t j = 1; j < ecount; j++) {
        q_pix[q_base + j - 1u] = x | (y << 16);
        q_cand[q_base + j - 1u] = cand_of((uint32_t)(clist >> (15u * j)) & 0x7FFFu);
    }
    uint32_t own_cxy = 0;
    if (ecount >= 1u) own_cxy = cand_of((uint32_t)clist & 0x7FFFu);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float own_corr = 0.0f;
    const unsigned long long idle = __ballot(ecount == 0u);
    const uint32_t n_idle = (uint32_t)__builtin_popcountll(idle);
    const uint32_t my_rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
    uint32_t done = 0;
    bool first_round = true;
    while (first_round || done < q_total) { // (wave-uniform; one round unless the queue is longer than the idle lanes are many)
        const bool own = first_round && ecount >= 1u;
        const uint32_t item = done + (first_round ? my_rank : lane);
        const bool take = !own && (!first_round || ecount == 0u) && item < q_total;
        uint32_t pxy = x | (y << 16), cxy = own_cxy;
        if (take) {
            pxy = q_pix[item];
            cxy = q_cand[item];
        }
        if (own || take) {
            const float corr = chain(pxy & 0xFFFFu, pxy >> 16, cxy & 0xFFFFu, cxy >> 16);
            exact_evals++;
            if (own) own_corr = corr;
            else q_corr[item] = corr;
        }
        done += first_round ? min(n_idle, q_total) : 64u;
        first_round = false;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (ecount >= 1u) consider(own_corr, (uint32_t)clist & 0x7FFFu, own_cxy);
    for (uint32_t j = 1; j < ecount; j++)
        consider(q_corr[q_base + j - 1u], (uint32_t)(clist >> (15u * j)) & 0x7FFFu, q_cand[q_base + j - 1u]);
    if (have) cell = make_uint2(bxy, __float_as_uint(bcorr));
    // (the pixel index again from the coordinates: kept across the walk and the chain it cost the lean instantiation a spill)
    uint32_t xs = x, ys = y;
    asm volatile("" : "+v"(xs), "+v"(ys));
    const size_t pix_e = (size_t)ys * p.w1 + xs;
    if (is_out && !whole) store_cell(p, out, out_score, pix_e, cell);
    if (counters) {
        uint32_t v0 = evaluated, v1 = exact_evals, v2 = ecount > 1u ? 1u : 0u, v3 = whole; // (v2: pixels with more than one contender)
        if (dbg & 32) { // diagnostics: displacements walked per wave (lean plan: after folding), waves that walked
            v1 = lane == 0 && wave_has ? (uint32_t)((mxx - mnx + 1 - fold_k) * NPL) : 0u;
            v2 = lane == 0 && wave_has ? 1u : 0u;
        }
#pragma unroll
        for (int sft = 32; sft > 0; sft >>= 1) {
            v0 += __shfl_down(v0, sft, 64);
            v1 += __shfl_down(v1, sft, 64);
            v2 += __shfl_down(v2, sft, 64);
            v3 += __shfl_down(v3, sft, 64);
        }
        if (COUNT && STEP && __any(bracket_missed) && lane == 0) atomicAdd(&counters[0], 1ull << 44);
        if (COUNT && ROWS && __any(row_mismatch) && lane == 0) atomicAdd(&counters[0], 1ull << 44); // (a candidate off the table's row)
        if (lane == 0) {
            if (v0) atomicAdd(&counters[0], (unsigned long long)v0);
            if (v1) atomicAdd(&counters[1], (unsigned long long)v1);
            if (v2) atomicAdd(&counters[2], (unsigned long long)v2);
            if (v3) atomicAdd(&counters[3], (unsigned long long)v3);
        }
    }
    {
        // Only a tile that goes onto the whole-corridor list has its contender words read (all of them: the settled
        // pixels' words must say so) - every other tile writes none: 8 B per pixel of HBM traffic less.
        const int any_whole = __syncthreads_or(whole ? 1 : 0);
        if (any_whole && is_out) contenders[pix_e] = word;
        if (threadIdx.x == 0 && any_whole)
            worklist_push(whole_list, TR ? (V0 | (tid.x << 16) | 0x40000000u) : ((uint32_t)U0 | (tid.y << 16)));
    }
#endif // BOX_STEP_SECTION
