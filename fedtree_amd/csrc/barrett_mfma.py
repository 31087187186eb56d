"""The matrix-core Barrett scheme that fthe_addb_q152 (gen_addb.py) and fthe_nadic_b76 (gen_nadicb.py) share, emitted
once: a product q c of 16 ciphertexts' bytes q (the B operands, 64-byte K-blocks in registers) with a constant c
(mu or the modulus) on v_mfma_i32_16x16x64_i8.  The A operand of output tile t (byte columns s_base + 16 t ..) and
K-block kb is a Toeplitz tile of c's balanced digits, read by one aligned ds_read_b128 per lane from one of 16
byte-shifted copies of c in LDS (row m's copy in slot copy_slot(m), byte KO + 16 (4 kb - t) + 16 h); the int32
accumulators start from the column corrections (srcC); each lane folds its four rows of a tile into an int64 group
that goes to a staging row in LDS, where the kernels' own signed normalisations pick the groups up.
tools/addb_model.py and tools/nadicb_model.py are the bit-exact models; barrett_image.hpp builds the copies and the
corrections on the host.  Plain functions: e is the caller's emit callback, o the list it appends to."""

M_A = (0, 1, 2, 3, 12, 13, 14, 15)           # rows whose copies sit in slots 0..7 (ds_read_b128 lane groups)
M_B = (4, 5, 6, 7, 8, 9, 10, 11)             # slots 8..15
LANE_MASK = {3: "s[20:21]", 0: "s[22:23]", 1: "s[24:25]", 2: "s[26:27]"}      # quad lane -> its lanes of the wave
XDL_WAIT = 19                                # wait states after an MFMA before a VALU reads its result


def pair(n):
    return f"v[{n}:{n + 1}]"


def quad4(n):
    return f"v[{n}:{n + 3}]"


def parse_switches(dbg, known, what):
    """the switch string (exact tokens between commas) or set -> frozenset of known switches"""
    toks = frozenset(t.strip() for t in dbg.split(',') if t.strip()) if isinstance(dbg, str) else frozenset(dbg)
    unknown = sorted(toks - set(known))
    if unknown:
        raise ValueError(f"unknown {what} switch {', '.join(unknown)}: known are {', '.join(known)}")
    return toks


# ---- tile geometry ---------------------------------------------------------------------------------------------
def copy_slot(m):
    return M_A.index(m) if m in M_A else 8 + M_B.index(m)


def band(nd, s0, k0):
    """the A tile of output bytes [s0, s0+16) x input bytes [k0, k0+64) has a nonzero digit c[s - k]"""
    lo, hi = s0 - k0 - 63, s0 + 15 - k0
    return not (hi < 0 or lo >= nd)


def active(nd, s_base, tiles, kbs):
    """per output tile, the K-blocks whose A tile is not all zero (the only MFMAs issued)"""
    return [[kb for kb in range(kbs) if band(nd, s_base + 16 * t, 64 * kb)] for t in range(tiles)]


# ---- prologue pieces ---------------------------------------------------------------------------------------------
def lane_masks(e):
    for j, pat in ((3, 0x88888888), (0, 0x11111111), (1, 0x22222222), (2, 0x44444444)):
        lo, hi = LANE_MASK[j][2:-1].split(':')
        e(f'  s_mov_b32 s{lo}, {hex(pat)}')
        e(f'  s_mov_b32 s{hi}, {hex(pat)}')


def fold_consts(e):
    """s30..s32: the byte weights of fold_tile; s33: the 0x80 bytes that turn u8 into i8 (b ^ 0x80 = b - 128)"""
    e('  s_movk_i32 s30, 0x100')
    e('  s_mov_b32 s31, 0x10000')
    e('  s_mov_b32 s32, 0x1000000')
    e('  s_mov_b32 s33, 0x80808080')


def image_to_lds(e, img_bytes, waves, lds_cnt, ctx, save, v_tid, v_row, v_ldsi, v_buf, v_tmp):
    """the key's constant image (ctx, img_bytes) -> LDS offset 0: every thread copies 16 B per pass, the last pass
    partial; then thread 0 clears the workgroup's batch counter at lds_cnt.  The caller waits and sets the barrier."""
    e(f'  v_lshlrev_b32_e32 v{v_row}, 4, v{v_tid}')
    per = 64 * waves * 16
    for off in range(0, img_bytes, per):
        part = off + per > img_bytes
        if part:
            e(f'  v_cmp_gt_u32_e32 vcc, {hex(img_bytes - off)}, v{v_row}')
            e(f'  s_and_saveexec_b64 {save}, vcc')
        e(f'  v_add_u32_e32 v{v_ldsi}, {hex(off)}, v{v_row}')
        e(f'  global_load_dwordx4 {quad4(v_buf)}, v{v_ldsi}, {ctx}')
        e('  s_waitcnt vmcnt(0)')
        e(f'  ds_write_b128 v{v_ldsi}, {quad4(v_buf)}')
        if part:
            e(f'  s_mov_b64 exec, {save}')
    e(f'  v_cmp_eq_u32_e32 vcc, 0, v{v_tid}')                              # thread 0: batch counter = 0
    e(f'  s_and_saveexec_b64 {save}, vcc')
    e(f'  v_mov_b32_e32 v{v_tmp}, {hex(lds_cnt)}')
    e(f'  v_mov_b32_e32 v{v_tmp + 1}, 0')
    e(f'  ds_write_b32 v{v_tmp}, v{v_tmp + 1}')
    e(f'  s_mov_b64 exec, {save}')


def copy_addrs(e, v_m, v_h16, v_a1, v_a2, v_c, copy, a2_off, corr1_off):
    """MFMA row m (v_m) and 16 h (v_h16) -> the lane's A read bases v_a1 (product 1: slot * COPY + 16 h, the copies
    from LDS offset 0), v_a2 (product 2) and its corrections base v_c.  The slot of row m, M_A -> 0..7, M_B ->
    8..15, is m < 4 ? m : m < 12 ? m + 4 : m - 8"""
    e(f'  v_add_u32_e32 v{v_a1}, 4, v{v_m}')
    e(f'  v_subrev_u32_e32 v{v_a2}, 8, v{v_m}')
    e(f'  v_cmp_gt_u32_e32 vcc, 12, v{v_m}')
    e(f'  v_cndmask_b32_e32 v{v_a1}, v{v_a2}, v{v_a1}, vcc')
    e(f'  v_cmp_gt_u32_e32 vcc, 4, v{v_m}')
    e(f'  v_cndmask_b32_e32 v{v_a1}, v{v_a1}, v{v_m}, vcc')
    e(f'  v_mul_u32_u24_e32 v{v_a1}, {copy}, v{v_a1}')
    e(f'  v_add_u32_e32 v{v_a1}, v{v_a1}, v{v_h16}')
    e(f'  v_add_u32_e32 v{v_a2}, {a2_off}, v{v_a1}')
    e(f'  v_add_u32_e32 v{v_c}, {corr1_off}, v{v_h16}')                    # + 64 t (+ CORR2 - CORR1)


# ---- the tile stream ---------------------------------------------------------------------------------------------
def lds_queue(e):
    """(issue, wait_for) over the outstanding LDS ops, oldest first: LDS returns in order, so s_waitcnt lgkmcnt(n)
    with n the ops issued after a tag's last one waits for exactly that op"""
    q = []

    def issue(tag, ins):
        e(ins)
        q.append(tag)

    def wait_for(tag):
        if tag in q:                             # else: completed with a later op already waited for
            i = len(q) - 1 - q[::-1].index(tag)
            e(f'  s_waitcnt lgkmcnt({min(len(q) - i - 1, 15)})')
            del q[:i + 1]
    return issue, wait_for


def settle(e, o, last):
    """wait states before a VALU read of accumulators whose last MFMA is o[last]: one per instruction issued since"""
    need = XDL_WAIT - sum(1 for ln in o[last + 1:] if ln.startswith('  '))
    while need > 0:
        e(f'  s_nop {min(need, 8) - 1}')
        need -= 8


def fold_tile(issue, e, tag, acc, pg, v_g, off):
    """acc's 4 int32 rows (output bytes 4h..4h+3 of the tile) -> the int64 group sum_i C_i 256^i -> LDS (v_g + off)"""
    e(f'  v_mad_i64_i32 {pair(pg)}, vcc, v{acc}, 1, 0')                   # sign-extended row 0
    e(f'  v_mad_i64_i32 {pair(pg)}, vcc, v{acc + 1}, s30, {pair(pg)}')
    e(f'  v_mad_i64_i32 {pair(pg)}, vcc, v{acc + 2}, s31, {pair(pg)}')
    e(f'  v_mad_i64_i32 {pair(pg)}, vcc, v{acc + 3}, s32, {pair(pg)}')
    issue(tag, f'  ds_write_b64 v{v_g}, {pair(pg)} offset:{off}')


def tile_ops(tiles, act):
    return [(n, t, kb) for n, t in enumerate(tiles) for kb in act[t]]


def read_a(issue, x, op, *, aop, v_a, ko, copy, **_):
    n, t, kb = op
    off = ko + 16 * (4 * kb - t)
    assert 0 <= off and off + 64 <= copy
    issue(('a', x), f'  ds_read_b128 {quad4(aop[x % 4])}, v{v_a} offset:{off}')


def read_corr(issue, n, t, *, accs, v_c, corr, **_):
    issue(('c', n), f'  ds_read_b128 {quad4(accs[n % len(accs)])}, v{v_c} offset:{corr + 64 * t}')


def first_reads(issue, tiles, act, **plan):
    """a stream's first corrections and A operands: constant image rows, independent of the q staging, so a stage
    may issue them ahead of its own writes (tile_stream(preloaded=True)) and overlap their round trip with it"""
    ops = tile_ops(tiles, act)
    for n in range(min(len(plan['accs']), len(tiles))):
        read_corr(issue, n, tiles[n], **plan)
    for x in range(min(3, len(ops))):
        read_a(issue, x, ops[x], **plan)


def tile_stream(e, o, tiles, act, stage, *, preloaded=False, mfma=True, **plan):
    """The MFMAs of the output tiles `tiles` (active K-blocks act[t]) as one stream, each tile folded into its int64
    groups at v_g + stage(t).  plan: accs (the accumulator sets), aop (four A-operand buffers), bq (the B operands,
    four registers per K-block), v_a (the A read base), ko, copy, v_c and corr (the corrections' base and offset),
    pg (the fold's pair), v_g.  A operands are read three MFMAs ahead into the four buffers (the buffer re-filled
    after MFMA x is MFMA x - 1's, whose operands were read at its issue).  With three accumulator sets tile n - 2
    is folded right after tile n's first MFMA, so its results have long been written (tile n - 1's MFMAs and reads
    in between) and the fold waits only for the wait states still missing (settle); tile n + 1's corrections
    (srcC, into the set tile n - 2 used) are read right after that fold.  preloaded: first_reads were issued and
    waited for by the caller.  mfma=False: the timing knock-out (wrong results).  Ends with the LDS drained."""
    accs, aop, bq = plan['accs'], plan['aop'], plan['bq']
    nacc = len(accs)
    ops = tile_ops(tiles, act)
    issue, wait_for = lds_queue(e)
    last_mfma = {}

    def fold(m):
        settle(e, o, last_mfma[m])
        fold_tile(issue, e, ('w', m), accs[m % nacc], plan['pg'], plan['v_g'], stage(tiles[m]))

    if not preloaded:
        first_reads(issue, tiles, act, **plan)
    for x, (n, t, kb) in enumerate(ops):
        first = x == 0 or ops[x - 1][0] != n
        if first:
            wait_for(('c', n))
        wait_for(('a', x))
        if mfma:
            acc = quad4(accs[n % nacc])
            e(f'  v_mfma_i32_16x16x64_i8 {acc}, {quad4(aop[x % 4])}, {quad4(bq + 4 * kb)}, {acc}')
        last_mfma[n] = len(o) - 1
        if x + 3 < len(ops):
            read_a(issue, x + 3, ops[x + 3], **plan)
        if first and n >= nacc - 1:
            m = n - (nacc - 1)
            fold(m)
            if m + nacc < len(tiles):
                read_corr(issue, m + nacc, tiles[m + nacc], **plan)
    for m in range(max(0, len(tiles) - (nacc - 1)), len(tiles)):
        fold(m)
    e('  s_waitcnt lgkmcnt(0)')
