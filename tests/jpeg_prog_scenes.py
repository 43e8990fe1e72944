"""The progressive JPEG files of the decoder's tests: (a) files that Pillow (libjpeg-turbo) writes with
progressive=True - libjpeg's default script has all four scan kinds -, (b) files from `write`, a small progressive writer
from quantised coefficients, a scan script and restart intervals, one DHT in front of every scan, which forces what an
encoder does not give on demand - SEAMS: the files that sit on the seams of the kernels' units -, and (c) the files that are
refused.  tests/test_jpeg_prog_ref.py checks that each forced file reaches its case."""
import functools

import numpy as np

import jpeg_scenes
import ref_jpeg
import ref_jpeg_prog
from jpeg_scenes import QUANT_PLAIN, _blocks, _picture, _small_coef, pillow_jpeg

SYNC_LANES = 256


# ---- (b) the writer ---------------------------------------------------------------------------------------------------------------
def _table_for(symbols, long_codes):
    """A DHT for exactly these symbols: one length for all (the code of all ones stays free), or 1 bit for the first and 16
    for the others."""
    symbols = sorted(symbols) or [0]
    if long_codes:
        return jpeg_scenes.table({s: 1 if k == 0 else 16 for k, s in enumerate(symbols)})
    return jpeg_scenes.table({s: max(2, len(symbols).bit_length()) for s in symbols})


def _magnitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


class _Tokens:
    """A restart interval as ("s", symbol) and ("b", value, bits) tokens, jcphuff.c's EOB run and correction-bit buffers."""

    def __init__(self):
        self.out, self.eobrun, self.pending = [], 0, []

    def symbol(self, s):
        self.out.append(("s", s))

    def bits(self, v, n):
        if n:
            self.out.append(("b", v, n))

    def flush_run(self):
        if self.eobrun:
            nbits = self.eobrun.bit_length() - 1
            self.symbol(nbits << 4)
            self.bits(self.eobrun & ((1 << nbits) - 1), nbits)
            self.eobrun = 0
        for b in self.pending:
            self.bits(b, 1)
        self.pending = []


def _encode_block(t, row, ss, se, ah, al, pred):
    """One block of one scan into t (row: natural order, DC value); -> the component's DC predictor."""
    zz = ref_jpeg.ZIGZAG
    if ss == 0:
        if ah:
            t.bits((row[0] >> al) & 1, 1)
            return pred
        v = row[0] >> al
        size, bits = _magnitude(v - pred)
        t.symbol(size)
        t.bits(bits, size)
        return v
    mags = [abs(row[zz[k]]) >> al for k in range(ss, se + 1)]
    if ah == 0:
        r = 0
        for k, mag in zip(range(ss, se + 1), mags):
            if mag == 0:
                r += 1
                continue
            t.flush_run()
            while r > 15:
                t.symbol(0xF0)
                r -= 16
            size = mag.bit_length()
            t.symbol(r << 4 | size)
            t.bits(mag if row[zz[k]] >= 0 else mag ^ ((1 << size) - 1), size)
            r = 0
        if r:
            t.eobrun += 1
            if t.eobrun == 0x7FFF:
                t.flush_run()
        return pred
    last_new = max([k for k, mag in zip(range(ss, se + 1), mags) if mag == 1], default=-1)
    r, br = 0, []
    for k, mag in zip(range(ss, se + 1), mags):
        if mag == 0:
            r += 1
            continue
        while r > 15 and k <= last_new:
            t.flush_run()
            t.symbol(0xF0)
            r -= 16
            for b in br:
                t.bits(b, 1)
            br = []
        if mag > 1:
            br.append(mag & 1)
            continue
        t.flush_run()
        t.symbol(r << 4 | 1)
        t.bits(0 if row[zz[k]] < 0 else 1, 1)
        for b in br:
            t.bits(b, 1)
        br, r = [], 0
    if r or br:
        t.eobrun += 1
        t.pending += br
        if t.eobrun == 0x7FFF or len(t.pending) > 937:
            t.flush_run()
    return pred


def write(width, height, coef, quant, script, sampling=(1, 1), components=3, restart=0, sof=0xC2, fill=0, eoi=True):
    """coef [blocks, 64] as jpeg_scenes.write takes them (DESIGN.md 4.16's block store, DC values); script: a list of scans
    dict(comps=[..], ss=, se=, ah=, al=, restart= (a DRI in front of the scan when it changes), long= (16-bit codes),
    encode_as= (the (Ah, Al) the entropy coding really uses, where the header is to lie)).  One DHT (slots 0) in front of every scan that needs one."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)

    hs, vs = sampling if components == 3 else (1, 1)
    frame = {"width": width, "height": height, "hmax": hs, "vmax": vs, "mcus_x": -(-width // (8 * hs)), "mcus_y": -(-height // (8 * vs)),
             "comps": [{"h": hs if c == 0 else 1, "v": vs if c == 0 else 1} for c in range(components)]}
    frame["first_slot"] = [0] + [hs * vs + c for c in range(components - 1)]
    frame["bpm"] = hs * vs + components - 1
    out = bytearray(b"\xff\xd8")
    out += seg(0xDB, bytes([0x00] + [quant[ref_jpeg.ZIGZAG[i]] for i in range(64)]))
    body = [8] + list(height.to_bytes(2, "big")) + list(width.to_bytes(2, "big")) + [components]
    for c in range(components):
        body += [c + 1, (sampling[0] << 4 | sampling[1]) if c == 0 else 0x11, 0]
    out += seg(sof, body)
    current = 0
    rows = [[int(v) for v in row] for row in coef]
    for scan in script:
        comps, ss, se, ah, al = scan["comps"], scan["ss"], scan["se"], scan["ah"], scan["al"]
        ri = scan.get("restart", restart)
        if ri != current:
            out += seg(0xDD, ri.to_bytes(2, "big"))
            current = ri
        enc_ah, enc_al = scan.get("encode_as", (ah, al))
        mcus, across = ref_jpeg_prog.scan_geometry(frame, comps)
        parts = []
        for first in range(0, mcus, ri or mcus):
            t = _Tokens()
            pred = {c: 0 for c in comps}
            for m in range(first, min(first + (ri or mcus), mcus)):
                for c, idx in ref_jpeg_prog.mcu_blocks(frame, comps, m, across):
                    pred[c] = _encode_block(t, rows[idx], ss, se, enc_ah, enc_al, pred[c])
            t.flush_run()
            parts.append(t.out)
        symbols = {tok[1] for part in parts for tok in part if tok[0] == "s"}
        tab = _table_for(symbols, scan.get("long", False))
        codes = jpeg_scenes._codes(tab)
        if symbols or not (ss == 0 and ah):
            out += seg(0xC4, [(0 if ss == 0 else 1) << 4] + tab[0] + tab[1])
        out += seg(0xDA, [len(comps)] + [v for c in comps for v in (c + 1, 0)] + [ss, se, ah << 4 | al])
        data = bytearray()
        for k, part in enumerate(parts):
            acc = "".join(format(codes[tok[1]][0], "0%db" % codes[tok[1]][1]) if tok[0] == "s" else format(tok[1], "0%db" % tok[2]) for tok in part)
            acc += "1" * (-len(acc) % 8)
            if k:
                data += b"\xff" * fill + bytes([0xFF, 0xD0 + ((k - 1) & 7)])
            data += bytes(int(acc[i:i + 8], 2) for i in range(0, len(acc), 8)).replace(b"\xff", b"\xff\x00")
        out += data
    if eoi:
        out += b"\xff" * fill + b"\xff\xd9"
    return bytes(out)


def S(comps, ss, se, ah, al, **more):
    return dict(comps=list(comps), ss=ss, se=se, ah=ah, al=al, **more)


def _bands(c, bands, al):
    """Component c's AC bands, each sent at `al` and refined down to 0, band by band."""
    return [S([c], a, b, ah, ah - 1 if ah else al) for a, b in bands for ah in ([0] + list(range(al, 0, -1)) if al else [0])]


def _script_mozjpeg(components):
    """DC scans per component, as mozjpeg writes them; bands 1-2, 3-9 and 10-63; Al = 3: three refinement passes."""
    out = []
    for c in range(components):
        out += [S([c], 0, 0, 0, 3)]
    for c in range(components):
        out += [S([c], 0, 0, ah, ah - 1) for ah in (3, 2, 1)]
    for c in range(components):
        out += _bands(c, [(1, 2), (3, 9), (10, 63)], 3)
    return out


def _script_y_then_chroma():
    """Y alone and then Cb + Cr together; spectral selection only; DRI changing between scans."""
    return [S([0], 0, 0, 0, 0, restart=2), S([1, 2], 0, 0, 0, 0, restart=3), S([0], 1, 5, 0, 0, restart=1), S([0], 6, 63, 0, 0, restart=0),
            S([1], 1, 63, 0, 0, restart=3), S([2], 1, 63, 0, 0, restart=3)]


def _script_default(components, al=1):
    """libjpeg's default script in small: interleaved DC, then each component's bands, then the refinements."""
    out = [S(range(components), 0, 0, 0, al)]
    for c in range(components):
        out += [S([c], 1, 5, 0, al + 1), S([c], 6, 63, 0, al + 1)]
    for c in range(components):
        out += [S([c], 1, 63, ah, ah - 1) for ah in range(al + 1, 0, -1)]
    return out + [S(range(components), 0, 0, ah, ah - 1) for ah in range(al, 0, -1)]


def _refine_coef(n, seed):
    """Blocks for the refinement cases, met in the last refinement (Al = 0) of the band 1 .. 63: block 0 - history (|v| >= 2) at 2 and 20, a new
    coefficient (|v| = 1) at 40, seventeen and more zero-history coefficients before it with the history inside (ZRL over
    history); block 1 - a new coefficient exactly at 63; block 2 - a new one at 5, history at 50 and 60 behind it (the band
    ends in history after the last new one); blocks 3 .. 5 - only history (an EOB run whose blocks read correction bits)."""
    zz = ref_jpeg.ZIGZAG
    coef = _small_coef(n, seed)
    coef[:6, 1:] = 0
    coef[0, zz[2]], coef[0, zz[20]], coef[0, zz[40]] = 6, -3, -1
    coef[1, zz[63]], coef[1, zz[7]] = 1, 2
    coef[2, zz[5]], coef[2, zz[50]], coef[2, zz[60]] = -1, 5, -2
    for b in (3, 4, 5):
        coef[b, zz[3 + b]], coef[b, zz[30]] = 3, -7
    return coef


def forced_mozjpeg_420():
    return write(33, 47, _small_coef(_blocks(33, 47, (2, 2)), 21), QUANT_PLAIN, _script_mozjpeg(3), sampling=(2, 2))


def forced_y_then_chroma_422():
    return write(21, 10, _small_coef(_blocks(21, 10, (2, 1)), 22), QUANT_PLAIN, _script_y_then_chroma(), sampling=(2, 1))


def forced_refine_444():
    """17 x 9 at 4:4:4, DRI 0: the refinement cases of _refine_coef in the luma blocks (blocks 0, 3, 6, .. of the store)."""
    n = _blocks(17, 9, (1, 1))
    coef = _small_coef(n, 23)
    coef[0::3][:6] = _refine_coef(6, 24)[:6]
    coef[15, 1:] = 0                                       # the scan's last luma block is inside an EOB run
    coef[12, 1:] = 0
    return write(17, 9, coef, QUANT_PLAIN, _script_default(3), sampling=(1, 1))


def forced_refine_grey_rst():
    """The same cases in a grey file with a restart interval of 4 blocks and FF FF fill in front of every marker."""
    n = _blocks(40, 24, (1, 1), 1)
    coef = _small_coef(n, 25)
    coef[:6] = _refine_coef(6, 26)[:6]
    coef[-2:, 1:] = 0
    return write(40, 24, coef, QUANT_PLAIN, _script_default(1), components=1, restart=4, fill=2)


def forced_codes16():
    n = _blocks(17, 9, (2, 2))
    return write(17, 9, _small_coef(n, 27), QUANT_PLAIN, [dict(s, long=True) for s in _script_default(3)], sampling=(2, 2))


def forced_eob16384():
    """1024 x 1024 grey, 16384 blocks without a non-zero AC coefficient: each AC scan is one EOB run of 16384 blocks (EOB14)."""
    coef = np.zeros((16384, 64), dtype=np.int64)
    coef[:, 0] = (np.arange(16384) * 7) % 200 - 100
    return write(1024, 1024, coef, QUANT_PLAIN, _script_default(1, al=0), components=1)


# ---- the seams of the kernels' units (Tests): 64-byte chunks and 256-lane workgroups of the byte kernels, 1024-bit
# subsequences 256 to a workgroup, a wave per restart interval, correction fields in 16-bit pieces.  Every seed below was found by
# the bounded search its builder still holds; the search starts at the seed written down, so a test pays for one try.
CHUNK, GROUP = 64, 256


def forced_dense_history():
    """48 x 16 grey, 12 blocks, every AC coefficient a history coefficient (|v| >= 2) of the band's last refinement (Al = 0) but for the
    exceptions: blocks 0, 1 - none, an EOB run of two whose blocks each read the whole band's 63 correction bits as one field, the
    second from inside the run; blocks 2 .. 8 - a new coefficient (|v| = 1) behind exactly 16, 17, 32, 33, 48, 49 and 62 history
    coefficients (the last at 63); block 9 - H H 0 sixteen times from 1 on, history to 54, a new coefficient at 55: the writer's ZRL
    runs over 16 zero-history positions with 32 history coefficients between them; block 10 - new coefficients behind fields of 16 and
    then 17; block 11 - none (the scan ends inside an EOB run)."""
    rng = np.random.RandomState(41)
    coef = np.zeros((12, 64), dtype=np.int64)
    coef[:, 0] = rng.randint(-60, 60, size=12)
    history = rng.choice([-1, 1], size=(12, 64)) * rng.randint(2, 8, size=(12, 64))
    for b in range(12):
        for k in range(1, 64):
            coef[b, ref_jpeg.ZIGZAG[k]] = history[b, k]
    for b, n in zip(range(2, 9), (16, 17, 32, 33, 48, 49, 62)):
        coef[b, ref_jpeg.ZIGZAG[n + 1]] = 1 if b & 1 else -1
    for k in range(3, 49, 3):
        coef[9, ref_jpeg.ZIGZAG[k]] = 0
    coef[9, ref_jpeg.ZIGZAG[55]] = -1
    coef[10, ref_jpeg.ZIGZAG[17]], coef[10, ref_jpeg.ZIGZAG[35]] = 1, -1
    return write(48, 16, coef, QUANT_PLAIN, _script_default(1), components=1)


DC_SLOTS = {"420": (128, (2, 2), 1), "422": (96, (2, 1), 8), "444": (80, (1, 1), 0)}   # sampling -> (size, factors, the seed found)


def _dc_slots_file(size, sampling, seed):
    coef = _small_coef(_blocks(size, size, sampling), seed)
    coef[:, 0] = np.random.RandomState(1000 + seed).randint(-1000, 1000, size=len(coef))
    return write(size, size, coef, QUANT_PLAIN, _script_default(3, al=0), sampling=sampling)


def _dc_entry_slots(data):
    met = {}
    ref_jpeg_prog.entropy_decode(ref_jpeg_prog.parse(data), met)
    return met["dc_entry_slots"]


def dc_slots_ok(slots, sampling):
    """At least three distinct slots at the subsequences' first blocks, a chroma slot among them and a luma slot above 0 (4:4:4 has
    the one luma slot: there the three are all there are)."""
    luma = sampling[0] * sampling[1]
    return len(slots) >= 3 and any(s >= luma for s, _ in slots) and (luma == 1 or any(0 < s < luma for s, _ in slots))


def forced_dc_slots(key):
    """size x size colour, DC values from -1000 .. 999 (differences of up to 11 bits), small AC; the interleaved DC-first scan is longer
    than three subsequences and their first blocks lie at three slots of the MCU at least: the first of 64 seeds from the one found."""
    size, sampling, first = DC_SLOTS[key]
    for seed in range(first, first + 64):
        data = _dc_slots_file(size, sampling, seed)
        if dc_slots_ok(_dc_entry_slots(data), sampling):
            return data
    raise AssertionError("no seed gives the slots")


def _rst_every_block_coef():
    return _small_coef(289, 43)


def forced_rst_every_block(fill=0):
    """136 x 136 grey, 17 x 17 blocks, DRI 1: 289 restart intervals in each of the 6 scans."""
    return write(136, 136, _rst_every_block_coef(), QUANT_PLAIN, _script_default(1), components=1, restart=1, fill=fill)


WIDE_FIRST = {False: (384, 0), True: (216, 5)}   # 16-bit codes or not -> (size, the seed found)


def _wide_first_file(size, seed, long_codes):
    """Half the blocks carry all 63 AC coefficients in -12 .. 12 without a zero, the others DC alone (EOB runs between them)."""
    rng = np.random.RandomState(seed)
    n = (size // 8) ** 2
    coef = np.zeros((n, 64), dtype=np.int64)
    coef[:, 0] = rng.randint(-60, 60, size=n)
    full = rng.randint(0, 2, size=n).astype(bool)
    values = rng.choice([-1, 1], size=(n, 63)) * rng.randint(1, 13, size=(n, 63))
    coef[full, 1:] = values[full]
    script = [dict(s, long=long_codes and s["ss"] > 0 and s["ah"] == 0) for s in _script_default(1)]
    return write(size, size, coef, QUANT_PLAIN, script, components=1)


def wide_first_seams(data):
    """The file's band 6 .. 63 first scan: (subsequences, a multiple of 256 of the first scans' lane order strictly inside one of
    its intervals, the three seam counts)."""
    h = ref_jpeg_prog.parse(data)
    met = {}
    ref_jpeg_prog.entropy_decode(h, met)
    k = [s[1:4] for s in met["scans"]].index((6, 63, 0))
    lane = sum(n for s, n in zip(met["scans"][:k], met["subsequences"][:k]) if s[3] == 0)   # (no DRI: an interval each)
    inside = any(lane < g < lane + met["subsequences"][k] for g in range(SYNC_LANES, lane + met["subsequences"][k], SYNC_LANES))
    return met["subsequences"][k], inside, tuple(met[key][k] for key in ("eob_run_ends_subsequence", "symbol_straddles_subsequence", "eobn_straddles_subsequence"))


def forced_wide_first(long_codes=False):
    size, first = WIDE_FIRST[long_codes]
    for seed in range(first, first + 64):
        data = _wide_first_file(size, seed, long_codes)
        subs, inside, counts = wide_first_seams(data)
        if subs > SYNC_LANES and inside and all(counts):
            return data
    raise AssertionError("no seed gives the seams")


def chunk_seams(data):
    """Where the bytes of the scans behind the first lie relative to the byte kernels' units, restated from the parsed file: virtual
    byte = the scan's vfirst (the running sum of the scans' lengths, each rounded up to 64, an empty scan 64) + the offset in the scan.
    -> the set of seams met: ("ff00" | "rst" | "fill", 64 | 256) for an FF 00 pair's FF, an RSTn's own FF, or a fill FF in front of an
    RSTn, as the last byte of a 64-byte chunk that ends no workgroup, or of a 256-byte workgroup; ("length", 0 | 1) for a scan of a
    multiple of 64 bytes, or one more."""
    h = ref_jpeg_prog.parse(data)
    met, vfirst = set(), 0
    for number, scan in enumerate(h["scans"]):
        s0, s1 = scan["range"]
        b = data[s0:s1]
        if number:
            if len(b) and len(b) % CHUNK in (0, 1):
                met.add(("length", len(b) % CHUNK))
            for i in range(len(b) - 1):
                v = vfirst + i
                if b[i] != 0xFF or v % CHUNK != CHUNK - 1:
                    continue
                unit = GROUP if v % GROUP == GROUP - 1 else CHUNK
                q = i + 1
                while q < len(b) and b[q] == 0xFF:
                    q += 1
                if b[i + 1] == 0:
                    met.add(("ff00", unit))
                elif 0xD0 <= b[i + 1] <= 0xD7:
                    met.add(("rst", unit))
                elif q < len(b) and 0xD0 <= b[q] <= 0xD7:
                    met.add(("fill", unit))
        vfirst += -(-len(b) // CHUNK) * CHUNK if len(b) else CHUNK
    return met


CHUNK_SEAMS = {("ff00", 64), ("ff00", 256), ("rst", 64), ("rst", 256), ("fill", 64), ("length", 0), ("length", 1)}
CHUNK_SEAMS_FILE = (9, 66)   # blocks across and down, the seed: what a search over sides 6 up, 300 seeds each, found first


def _chunk_seams_file(side, seed):
    """side x side grey blocks, DRI 1, FF FF fill: an interval of a DC-refinement scan is one bit and seven pad bits, the byte 7F, or FF 00
    where the bit is set, so the two low bits of the DC values lay out the two DC-refinement scans (Al = 1 and 0) byte by byte; they
    are random by the seed, and the last blocks' are then set or cleared until the scan's length is 0, and the last scan's 1, modulo 64
    (the last scan holds the two fill bytes in front of EOI)."""
    n = side * side
    rng = np.random.RandomState(seed)
    coef = _small_coef(n, 49)
    coef[:, 1:] *= 4   # (the AC first scans are at Al = 3)
    low = rng.randint(0, 2, size=(2, n))
    for row, want, tail in ((low[0], 0, 0), (low[1], 1, 2)):
        length = lambda: n + int(row.sum()) + 4 * (n - 1) + tail   # noqa: E731
        more = (want - length()) % CHUNK
        flip, value = (more, 1) if more <= n - int(row.sum()) else (CHUNK - more, 0)   # (where neither can be had the search goes on)
        row[[k for k in range(n - 1, -1, -1) if row[k] != value][:flip]] = value
    coef[:, 0] = 4 * rng.randint(-15, 15, size=n) + 2 * low[0] + low[1]
    return write(8 * side, 8 * side, coef, QUANT_PLAIN, _script_default(1, al=2), components=1, restart=1, fill=2)


def forced_chunk_seams():
    side, first = CHUNK_SEAMS_FILE
    for seed in range(first, first + 10000):
        data = _chunk_seams_file(side, seed)
        if chunk_seams(data) >= CHUNK_SEAMS:
            return data
    raise AssertionError("no seed gives the seams")


def forced_mozjpeg_420_rst(restart):
    return write(33, 47, _small_coef(_blocks(33, 47, (2, 2)), 21), QUANT_PLAIN, _script_mozjpeg(3), sampling=(2, 2), restart=restart)


REFINE_TAILS = [8 * n - 3 for n in range(1, 18)] + [8, 64, 72, 128, 136]   # the bits of each block's interval in the last refinement


def forced_refine_tails():
    """One row of 22 grey blocks, DRI 1.  Block b's coefficients 1 .. m are all non-zero, new ones (|v| = 1: a 2-bit code and a sign)
    and history (|v| = 2, 3: a correction bit), the last of them history, then zeros: the interval of the last refinement (Al = 0) is
    3 new + history + 2 (EOB) bits long, REFINE_TAILS[b] - 1 .. 17 bytes, and five of them end on their last correction bit."""
    rng = np.random.RandomState(47)
    coef = np.zeros((len(REFINE_TAILS), 64), dtype=np.int64)
    coef[:, 0] = rng.randint(-60, 60, size=len(coef))
    for b, bits in enumerate(REFINE_TAILS):
        new = max(0, -(-(bits - 2 - 62) // 2))   # 3 new + history = bits - 2 in at most 62 positions ...
        new += int(rng.randint(0, (bits - 3) // 3 - new + 1))   # ... and a history coefficient at least
        kinds = [1] * new + [0] * (bits - 2 - 3 * new - 1)
        rng.shuffle(kinds)
        for k, is_new in enumerate(kinds + [0], 1):
            coef[b, ref_jpeg.ZIGZAG[k]] = int(rng.choice([-1, 1])) * (1 if is_new else int(rng.randint(2, 4)))
    return write(8 * len(coef), 8, coef, QUANT_PLAIN, _script_default(1), components=1, restart=1)


AL_HIGH = (5, 6)   # the Al of the DC's and of the AC bands' first scans


def forced_al_high():
    """32 x 32 grey: the rounded forward DCT of a two-level noise picture under a quantisation table of ones - an encoder's magnitudes, up to
    category 9 -, the DC sent at Al = 5 and refined five times, the AC bands at Al = 6 and refined six times."""
    k = np.arange(8)
    d = np.sqrt(0.25) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
    d[0] = np.sqrt(0.125)
    pixels = np.random.RandomState(48).choice([0.0, 255.0], size=(32, 32)) - 128   # two-level noise: AC magnitudes past 255
    coef = np.array([np.rint(d @ pixels[y:y + 8, x:x + 8] @ d.T).reshape(64) for y in range(0, 32, 8) for x in range(0, 32, 8)]).astype(np.int64)
    dc_al, ac_al = AL_HIGH
    script = [S([0], 0, 0, 0, dc_al), S([0], 1, 5, 0, ac_al), S([0], 6, 63, 0, ac_al)]
    script += [S([0], 1, 63, ah, ah - 1) for ah in range(ac_al, 0, -1)] + [S([0], 0, 0, ah, ah - 1) for ah in range(dc_al, 0, -1)]
    return write(32, 32, coef, [1] * 64, script, components=1)


FORCED = {"p_mozjpeg_420": forced_mozjpeg_420, "p_y_then_chroma_422": forced_y_then_chroma_422, "p_refine_444": forced_refine_444,
          "p_refine_grey_rst": forced_refine_grey_rst, "p_codes16": forced_codes16, "p_eob16384": forced_eob16384}
SEAMS = {"p_dense_history": forced_dense_history, "p_dc_slots_420": lambda: forced_dc_slots("420"), "p_dc_slots_422": lambda: forced_dc_slots("422"),
         "p_dc_slots_444": lambda: forced_dc_slots("444"), "p_rst_every_block": forced_rst_every_block,
         "p_rst_every_block_fill": lambda: forced_rst_every_block(fill=1), "p_wide_first": forced_wide_first,
         "p_wide_first_codes16": lambda: forced_wide_first(True), "p_mozjpeg_420_rst5": lambda: forced_mozjpeg_420_rst(5),
         "p_mozjpeg_420_rst1": lambda: forced_mozjpeg_420_rst(1), "p_refine_tails": forced_refine_tails, "p_al_high": forced_al_high,
         "p_chunk_seams": forced_chunk_seams}
FORCED.update(SEAMS)
# the writer's files with every coefficient sent down to Al = 0: the same coefficients make a baseline file
COEFFICIENTS = {
    "p_mozjpeg_420": lambda: (33, 47, _small_coef(_blocks(33, 47, (2, 2)), 21), dict(sampling=(2, 2))),
    "p_y_then_chroma_422": lambda: (21, 10, _small_coef(_blocks(21, 10, (2, 1)), 22), dict(sampling=(2, 1))),
    "p_codes16": lambda: (17, 9, _small_coef(_blocks(17, 9, (2, 2)), 27), dict(sampling=(2, 2))),
}


# ---- (a) Pillow's files ------------------------------------------------------------------------------------------------------------
def _pillow(w, h, kind, seed=0, grey=False, **options):
    return pillow_jpeg(_picture(w, h, kind, seed), grey=grey, progressive=True, **options)


@functools.lru_cache(maxsize=None)
def noise_size():
    """The smallest multiple of 8 at which Pillow's progressive file of size x size grey noise (quality 95, no DRI) has an
    AC-first scan of more than 256 subsequences (tests/test_jpeg_prog_ref.py asserts that one below has none)."""
    for size in range(64, 513, 8):
        if _most_first_subsequences(_pillow(size, size, "noise", grey=True, quality=95)) > SYNC_LANES:
            return size
    raise AssertionError("no size gives the subsequences")


def _most_first_subsequences(data):
    h = ref_jpeg_prog.parse(data)
    most = 0
    for scan in h["scans"]:
        if scan["ss"] > 0 and scan["ah"] == 0:
            most = max(most, sum(max(1, -(-8 * len(seg) // ref_jpeg_prog.SUBSEQ_BITS)) for seg, _ in ref_jpeg_prog.intervals(h["data"], scan)))
    return most


ENCODED = {
    "q_1x1_420": lambda: _pillow(1, 1, "smooth", quality=95, subsampling=2),
    "q_8x8_444": lambda: _pillow(8, 8, "smooth", quality=50, subsampling=0),
    "q_8x8_grey": lambda: _pillow(8, 8, "noise", grey=True, quality=95),
    "q_17x9_444": lambda: _pillow(17, 9, "noise", quality=95, subsampling=0),
    "q_17x9_422": lambda: _pillow(17, 9, "smooth", quality=50, subsampling=1),
    "q_17x9_420": lambda: _pillow(17, 9, "noise", quality=50, subsampling=2),
    "q_17x9_grey_rst1": lambda: _pillow(17, 9, "noise", grey=True, quality=50, restart_marker_blocks=1),
    "q_33x47_444_rst3": lambda: _pillow(33, 47, "smooth", 1, quality=50, subsampling=0, restart_marker_blocks=3),
    "q_33x47_422_rst1": lambda: _pillow(33, 47, "noise", quality=95, subsampling=1, restart_marker_blocks=1),
    "q_33x47_420": lambda: _pillow(33, 47, "smooth", quality=95, subsampling=2),
    "q_33x47_420_rst3": lambda: _pillow(33, 47, "noise", quality=50, subsampling=2, restart_marker_blocks=3),
    "q_33x47_grey": lambda: _pillow(33, 47, "smooth", grey=True, quality=95),
    "q_exif": lambda: _pillow(24, 16, "smooth", quality=90, subsampling=2, exif=b"Exif\0\0" + jpeg_scenes.exif_bytes(28)),
    "q_noise_grey": lambda: _pillow(noise_size(), noise_size(), "noise", grey=True, quality=95),
    "q_flat256_420": lambda: _pillow(256, 256, "flat", quality=90, subsampling=2),
}
FOCAL = {"q_exif": 28}
IN_ENCODER_RANGE = ("p_mozjpeg_420", "p_y_then_chroma_422", "p_refine_444", "p_refine_grey_rst", "p_codes16", "p_eob16384") + tuple(sorted(SEAMS))


def names():
    return sorted(ENCODED) + sorted(FORCED)


@functools.lru_cache(maxsize=None)
def scene(name):
    return (ENCODED.get(name) or FORCED[name])()


@functools.lru_cache(maxsize=None)
def restated(name):
    """The file's pixels by tests/ref_jpeg_prog.py: {"rgb", "luma", "met"}; computed once and left unchanged."""
    met = {}
    h = ref_jpeg_prog.parse(scene(name))
    coef, _ = ref_jpeg_prog.entropy_decode(h, met)
    rgb, luma = ref_jpeg_prog.pixels_of(h, coef, ref_jpeg_prog.RGB8), ref_jpeg_prog.pixels_of(h, coef, ref_jpeg_prog.LUMA8)
    rgb.setflags(write=False)
    luma.setflags(write=False)
    return {"rgb": rgb, "luma": luma, "met": met}


# ---- (c) the refused files ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refused():
    """name -> (file, code)."""
    U, I = ref_jpeg.UNSUPPORTED, ref_jpeg.INVALID
    n = _blocks(17, 9, (1, 1))
    coef = _small_coef(n, 31)

    def w(script, **more):
        return write(17, 9, coef, QUANT_PLAIN, script, **more)

    dc = [S(range(3), 0, 0, 0, 0)]
    full = dc + [S([c], 1, 63, 0, 0) for c in range(3)]
    out = {
        "dc_only": (w(dc), U),
        "ac_1_5_never_sent": (w(dc + [S([c], 6, 63, 0, 0) for c in range(3)]), U),
        "ac_left_at_al1": (w(dc + [S([c], 1, 63, 0, 1) for c in range(3)]), U),
        "ah_mismatch": (w(dc + [S([0], 1, 63, 0, 2), S([0], 1, 63, 1, 0)] + [S([c], 1, 63, 0, 0) for c in (1, 2)]), I),
        "ac_before_dc": (w([S([0], 1, 63, 0, 0)] + full), I),
        "ss_above_se": (w(dc + [S([0], 9, 5, 0, 0)] + full[1:]), I),
        "ac_two_components": (w(dc + [S([0, 1], 1, 63, 0, 0)] + full[1:]), I),
        "sof0_two_scans": (w(full, sof=0xC0), U),
        "baseline": (jpeg_scenes.scene("e_17x9_420"), U),
    }
    # s = 2 in a refinement: Y's band sent at Al = 1, then a scan that says Ah = 1 but is coded as a first scan, whose first
    # symbol is (0, 2) for a coefficient of 3
    big = coef.copy()
    big[0, 1] = 3
    out["refinement_s2"] = (write(17, 9, big, QUANT_PLAIN, dc + [S([0], 1, 63, 0, 1), S([0], 1, 63, 1, 0, encode_as=(0, 0))]
                                  + [S([c], 1, 63, 0, 0) for c in (1, 2)]), I)
    # a misnumbered and a missing RSTn, in the first scan that has one
    rst = scene("q_33x47_422_rst1")
    k = rst.index(b"\xff\xd1", rst.index(b"\xff\xda"))
    out["misnumbered_rst"] = (rst[:k + 1] + b"\xd3" + rst[k + 2:], I)
    out["missing_rst"] = (rst[:k] + rst[k + 2:], I)
    good = w(full)
    body = good.rindex(b"\xff\xda") + 10   # the last scan's first entropy byte
    out["scan_cut_short"] = (good[:body + (len(good) - 2 - body) // 2], I)
    return out


def _scan_range(data, ss, ah, al):
    return next(s["range"] for s in ref_jpeg_prog.parse(data)["scans"] if (s["ss"], s["ah"], s["al"]) == (ss, ah, al))


REFUSED_SEAMS = ("cut_in_a_63_bit_field", "cut_on_a_subsequence_boundary", "misnumbered_rst_257")   # refused_seams()'s names, without building it


@functools.lru_cache(maxsize=None)
def refused_seams():
    """name -> (file, code): the seam scenes broken at their seams; the scans behind the broken one stay, so the progression is whole."""
    out = {}
    # the band's last refinement cut 4 bytes in: an EOB1 code, its bit, and the data ends inside block 0's 63-bit correction field
    dense = scene("p_dense_history")
    s0, s1 = _scan_range(dense, 1, 1, 0)
    assert 0xFF not in dense[s0:s0 + 4]
    out["cut_in_a_63_bit_field"] = (dense[:s0 + 4] + dense[s1:], ref_jpeg.INVALID)
    # the band 6 .. 63 first scan cut behind half its data bytes rounded down to a multiple of 128: the data ends on a subsequence
    # boundary with blocks missing
    wide = scene("p_wide_first")
    s0, s1 = _scan_range(wide, 6, 0, 2)
    clean = len(wide[s0:s1].replace(b"\xff\x00", b"\xff"))
    want, at, seen = clean // 2 // 128 * 128, s0, 0
    while seen < want:
        at += 2 if wide[at] == 0xFF else 1
        seen += 1
    assert want >= 128 * SYNC_LANES // 2 and len(wide[s0:at].replace(b"\xff\x00", b"\xff")) == want
    out["cut_on_a_subsequence_boundary"] = (wide[:at] + wide[s1:], ref_jpeg.INVALID)
    # marker 257 (counted from 0: RST1) of the fourth scan numbered RST2
    rst = scene("p_rst_every_block")
    s0, s1 = ref_jpeg_prog.parse(rst)["scans"][3]["range"]
    markers = [i for i in range(s0, s1 - 1) if rst[i] == 0xFF and 0xD0 <= rst[i + 1] <= 0xD7]
    assert len(markers) == 288 and rst[markers[257] + 1] == 0xD1
    out["misnumbered_rst_257"] = (rst[:markers[257] + 1] + b"\xd2" + rst[markers[257] + 2:], ref_jpeg.INVALID)
    assert tuple(sorted(out)) == REFUSED_SEAMS
    return out
