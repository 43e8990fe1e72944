"""The definition of cvhip_jpeg_progressive_decode's pixels, restated sequentially in Python: the marker walk
over every scan of a progressive (SOF2) file, the progression checks with a ledger of the Al every coefficient was last sent
with, the four entropy codings of T.81 G.1 as libjpeg's jdphuff.c decodes them (DC first, DC refinement, AC first with EOB
runs, AC refinement with its correction bits), and the coefficients accumulated over all scans in DESIGN.md 4.16's block
store.  From there the pixels are ref_jpeg's: dequantisation, jidctint in 64-bit integers, fancy upsampling, YCbCr -> RGB and
the luma rule, unchanged.

Pinned: the RGB8 of an encoder-made progressive file equals Pillow's (libjpeg-turbo's) `convert("RGB")` byte for byte
(tests/test_jpeg_prog_ref.py).  A progression that leaves one of a component's coefficients 0 .. 9 unsent or unrefined is
refused (UNSUPPORTED): there libjpeg smooths between blocks, differently from version to version; inside the rule it never
does.  Where a file does what an encoder does not (a run past Se, s > 1 in a refinement) this file is the definition."""
import numpy as np

import ref_jpeg
from ref_jpeg import INVALID, LUMA8, RGB8, UNSUPPORTED, ZIGZAG, JpegError, _fail  # noqa: F401  (the codes are this module's too)

SUBSEQ_BITS = 1024   # jpeg_common.hpp's SUBSEQ_BITS: the unit `met` counts a scan's bits in
MAX_SCANS = 256
PAD = b"\xff" * 320  # behind an interval's bytes: a block reads at most 64 symbols of at most 32 bits past its end before the check


def _dqt(seg, quant):
    k = 0
    while k < len(seg):
        pq, tq = seg[k] >> 4, seg[k] & 15
        if pq > 1 or tq > 3 or k + 1 + 64 * (pq + 1) > len(seg):
            _fail(INVALID, "DQT")
        vals = [seg[k + 1 + i] if pq == 0 else seg[k + 1 + 2 * i] << 8 | seg[k + 2 + 2 * i] for i in range(64)]
        table = [0] * 64
        for i in range(64):
            table[ZIGZAG[i]] = vals[i]
        quant[tq] = table
        k += 1 + 64 * (pq + 1)


def _dht(seg, huff):
    k = 0
    while k < len(seg):
        if k + 17 > len(seg):
            _fail(INVALID, "DHT")
        tc, th = seg[k] >> 4, seg[k] & 15
        counts = list(seg[k + 1:k + 17])
        total = sum(counts)
        if tc > 1 or th > 3 or total > 256 or k + 17 + total > len(seg):
            _fail(INVALID, "DHT")
        symbols = list(seg[k + 17:k + 17 + total])
        code, s, lut = 0, 0, np.zeros(65536, dtype=np.uint16)
        for bits in range(1, 17):
            for _ in range(counts[bits - 1]):
                if code >= (1 << bits):
                    _fail(INVALID, "DHT: the code space is overfull")
                if tc == 0 and symbols[s] > 15:
                    _fail(INVALID, "DHT: a DC category above 15")
                lut[code << (16 - bits):(code + 1) << (16 - bits)] = bits << 8 | symbols[s]
                code, s = code + 1, s + 1
            code <<= 1
        huff[(tc, th)] = {"counts": counts, "symbols": symbols, "lut": lut}   # (a new object: a scan keeps the table it saw)
        k += 17 + total


def _scan_end(data, start):
    """The first FF at or behind `start` that is followed by neither 00, FF nor RSTn, or the file's end (ref_jpeg.parse)."""
    n, end = len(data), start
    while end < n:
        end = data.find(b"\xff", end)
        if end < 0 or end + 1 >= n:
            return n
        nx = data[end + 1]
        if nx == 0 or nx == 0xFF or 0xD0 <= nx <= 0xD7:
            end += 1 if nx == 0xFF else 2
            continue
        break
    return end


def scan_geometry(frame, comps):
    """-> (the scan's MCUs, blocks across of a single-component scan).  Several components: the frame's MCUs.  One: the
    component's own ceil(dw / 8) x ceil(dh / 8) blocks in raster order."""
    if len(comps) > 1:
        return frame["mcus_x"] * frame["mcus_y"], 0
    c = frame["comps"][comps[0]]
    dw, dh = -(-frame["width"] * c["h"] // frame["hmax"]), -(-frame["height"] * c["v"] // frame["vmax"])
    return -(-dw // 8) * -(-dh // 8), -(-dw // 8)


def mcu_blocks(frame, comps, m, across):
    """The blocks of scan MCU m in coding order as (component, index into DESIGN.md 4.16's block store)."""
    bpm, first = frame["bpm"], frame["first_slot"]
    if len(comps) == 1:
        c = comps[0]
        ch, cv = frame["comps"][c]["h"], frame["comps"][c]["v"]
        bx, by = m % across, m // across
        return [(c, ((by // cv) * frame["mcus_x"] + bx // ch) * bpm + first[c] + (by % cv) * ch + bx % ch)]
    return [(c, m * bpm + first[c] + q) for c in comps for q in range(frame["comps"][c]["h"] * frame["comps"][c]["v"])]


def parse(data):
    """The marker walk over the whole file -> the frame and the scan list.  Raises JpegError(INVALID | UNSUPPORTED)."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        _fail(INVALID, "no SOI")
    at = 2
    quant, huff, frame, restart, focal, adobe, scans = {}, {}, None, 0, 0, None, []
    ledger = None
    while True:
        if at >= n:
            if scans:
                break   # (no EOI: the file's end is the end, as for a baseline file's scan)
            _fail(INVALID, "no marker")
        if data[at] != 0xFF:
            _fail(INVALID, "no marker")
        while at < n and data[at] == 0xFF:
            at += 1
        if at >= n:
            if scans:
                break
            _fail(INVALID, "the file ends in a marker")
        m = data[at]
        at += 1
        if m == 0xD9 and scans:
            break
        if m == 0xD9 or m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x00:
            _fail(INVALID, "marker %02X outside a scan" % m)
        if m == 0x01:
            continue
        if at + 2 > n:
            _fail(INVALID, "truncated segment")
        length = data[at] << 8 | data[at + 1]
        if length < 2 or at + length > n:
            _fail(INVALID, "truncated segment")
        seg = data[at + 2:at + length]
        if m == 0xDB:
            _dqt(seg, quant)
        elif m == 0xC4:
            _dht(seg, huff)
        elif m == 0xDD:
            if len(seg) != 2:
                _fail(INVALID, "DRI")
            restart = seg[0] << 8 | seg[1]
        elif m == 0xC2:
            if frame is not None:
                _fail(INVALID, "two frames")
            if len(seg) < 6:
                _fail(INVALID, "SOF")
            p, h, w, nf = seg[0], seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            if len(seg) != 6 + 3 * nf:
                _fail(INVALID, "SOF")
            if p == 12:
                _fail(UNSUPPORTED, "12-bit")
            if p != 8:
                _fail(INVALID, "precision")
            if h == 0:
                _fail(UNSUPPORTED, "DNL")
            if w == 0:
                _fail(INVALID, "width 0")
            if nf in (2, 4):
                _fail(UNSUPPORTED, "2 or 4 components")
            if nf not in (1, 3):
                _fail(INVALID, "components")
            comps = [{"id": seg[6 + 3 * c], "h": seg[7 + 3 * c] >> 4, "v": seg[7 + 3 * c] & 15, "tq": seg[8 + 3 * c]} for c in range(nf)]
            for c in comps:
                if not 1 <= c["h"] <= 4 or not 1 <= c["v"] <= 4 or c["tq"] > 3:
                    _fail(INVALID, "SOF")
            if nf == 1:
                comps[0]["h"] = comps[0]["v"] = 1
            elif (comps[0]["h"], comps[0]["v"]) not in ((1, 1), (2, 1), (2, 2)) or any((c["h"], c["v"]) != (1, 1) for c in comps[1:]):
                _fail(UNSUPPORTED, "sampling")
            hmax, vmax = comps[0]["h"], comps[0]["v"]
            first, slot = [], 0
            for c in comps:
                first.append(slot)
                slot += c["h"] * c["v"]
            frame = {"width": w, "height": h, "comps": comps, "hmax": hmax, "vmax": vmax, "mcus_x": -(-w // (8 * hmax)),
                     "mcus_y": -(-h // (8 * vmax)), "bpm": slot, "first_slot": first}
            ledger = [[-1] * 64 for _ in comps]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            _fail(UNSUPPORTED, "SOF%d: not a progressive frame" % (m - 0xC0))   # (a baseline file too: cvhip_jpeg_decode's)
        elif m == 0xCC:
            _fail(UNSUPPORTED, "arithmetic conditioning")
        elif m == 0xDC:
            _fail(UNSUPPORTED, "DNL")
        elif m == 0xE1 and seg[:6] == b"Exif\0\0" and focal == 0:
            focal = ref_jpeg.exif_focal_length_35mm(seg[6:])
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                _fail(INVALID, "a scan before the frame")
            if len(scans) >= MAX_SCANS:
                _fail(UNSUPPORTED, "more than 256 scans")
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                _fail(INVALID, "SOS")
            ns = seg[0]
            if ns < 1 or ns > len(frame["comps"]):
                _fail(INVALID, "SOS")
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            if ss > se or se > 63 or (ss == 0 and se != 0) or (ss > 0 and ns != 1) or al > 13 or ah > 13:
                _fail(INVALID, "SOS: the band or the bit position")
            if ah and al != ah - 1:
                _fail(INVALID, "SOS: a refinement of more than one bit")
            if len(frame["comps"]) == 3 and adobe is not None and adobe != 1:
                _fail(UNSUPPORTED, "an Adobe transform that is not YCbCr")
            comps, dc, ac = [], {}, None
            for k in range(ns):
                ids = [c["id"] for c in frame["comps"]]
                if seg[1 + 2 * k] not in ids:
                    _fail(INVALID, "SOS: no such component")
                c = ids.index(seg[1 + 2 * k])
                if comps and c <= comps[-1]:
                    _fail(INVALID, "SOS: the components are not in the frame's order")
                td, ta = seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15
                if td > 3 or ta > 3:
                    _fail(INVALID, "SOS")
                comp = frame["comps"][c]
                if "quant" not in comp:   # (libjpeg latches a component's table at its first scan)
                    if comp["tq"] not in quant:
                        _fail(INVALID, "a missing table")
                    comp["quant"] = quant[comp["tq"]]
                if ss == 0 and ah == 0:
                    if (0, td) not in huff:
                        _fail(INVALID, "a missing table")
                    dc[c] = huff[(0, td)]
                if ss > 0:
                    if (1, ta) not in huff:
                        _fail(INVALID, "a missing table")
                    ac = huff[(1, ta)]
                    if ledger[c][0] < 0:
                        _fail(INVALID, "an AC scan before the component's DC scan")
                for z in range(ss, se + 1):
                    if ah == 0 and ledger[c][z] >= 0:
                        _fail(INVALID, "a first scan of coefficients that were sent")
                    if ah and ledger[c][z] != ah:
                        _fail(INVALID, "Ah is not the Al the coefficients were last sent with")
                    ledger[c][z] = al
                comps.append(c)
            start = at + length
            end = _scan_end(data, start)
            mcus, across = scan_geometry(frame, comps)
            scans.append({"comps": comps, "ss": ss, "se": se, "ah": ah, "al": al, "restart": restart, "range": (start, end), "dc": dc, "ac": ac,
                          "mcus": mcus, "across": across, "intervals": -(-mcus // restart) if restart else 1})
            at = end
            continue
        at += length
    for c, comp in enumerate(frame["comps"]):
        if any(ledger[c][z] != 0 for z in range(10)):
            _fail(UNSUPPORTED, "an incomplete progression: a coefficient 0 .. 9 is unsent or unrefined")
    return {**frame, "scans": scans, "focal_length_35mm": focal, "data": data, "ledger": ledger}


def info(data):
    h = parse(data)
    return {"width": h["width"], "height": h["height"], "components": len(h["comps"]), "h": h["hmax"], "v": h["vmax"],
            "focal_length_35mm": h["focal_length_35mm"], "scans": len(h["scans"])}


def intervals(data, scan):
    """The scan's bytes cut at its RSTn markers -> per restart interval its unstuffed bytes and its (begin, end) in the file,
    end at the marker's first FF.  A run of FF bytes is a data byte FF when 00 follows it, a marker when RSTn does, and the
    end of the data where the range ends."""
    s0, s1 = scan["range"]
    want = scan["intervals"]
    out, cur, i, begin = [], bytearray(), s0, s0
    while i < s1:
        b = data[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        q = i + 1
        while q < s1 and data[q] == 0xFF:
            q += 1
        if q >= s1:
            break
        if data[q] == 0:
            cur.append(0xFF)
            i = q + 1
            continue
        if data[q] != 0xD0 + (len(out) & 7) or len(out) + 1 >= want:  # (0xD0 .. 0xD7 by the scan's range)
            _fail(INVALID, "a misnumbered or surplus RSTn")
        out.append((bytes(cur), (begin, i)))
        cur, i, begin = bytearray(), q + 1, q + 1
    out.append((bytes(cur), (begin, i)))
    if len(out) != want:
        _fail(INVALID, "a missing RSTn")
    return out


class _Bits:
    def __init__(self, seg, met):
        self.buf, self.p, self.nbits, self.met, self.last_correction = seg + PAD, 0, 8 * len(seg), met, -1

    def get(self, n):
        if n == 0:
            return 0
        i = self.p >> 3
        w = int.from_bytes(self.buf[i:i + 4], "big")
        v = (w >> (32 - (self.p & 7) - n)) & ((1 << n) - 1)
        self.p += n
        return v

    def symbol(self, lut):
        i = self.p >> 3
        w = int.from_bytes(self.buf[i:i + 4], "big")
        e = lut[(w >> (16 - (self.p & 7))) & 0xFFFF]
        if e == 0:
            _fail(INVALID, "a code that is not in its table")
        self.p += e >> 8
        if (e >> 8) > self.met["longest_code"]:
            self.met["longest_code"] = e >> 8
        return e & 255


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _refine_block(bits, row, ss, se, al, lut, eobrun, met):
    """decode_mcu_AC_refine of jdphuff.c for one block (row: the block's 64 coefficients, natural order) -> EOBRUN."""
    p1 = 1 << al
    k = ss
    entered_in_run = eobrun > 0
    placed = False

    def correct(z):
        v = row[z]
        bit = bits.get(1)
        bits.last_correction = bits.p
        if bit and (v & p1):
            met["correction_on_set_bit"] += 1
        if bit and (v & p1) == 0:
            row[z] = _wrap16(v + p1 if v >= 0 else v - p1)

    def field(n):   # what correct_wave reads at once: the corrections between the walk's position and its target
        if n:
            met["correction_field_bits"].add(n)

    if eobrun == 0:
        while k <= se:
            sym = bits.symbol(lut)
            r, s = sym >> 4, sym & 15
            value = 0
            if s:
                if s != 1:
                    _fail(INVALID, "a refinement symbol of more than one bit")
                value = p1 if bits.get(1) else -p1   # (the sign comes before the position is walked)
            elif r != 15:
                eobrun = (1 << r) + bits.get(r)
                met["longest_eob_run"] = max(met["longest_eob_run"], eobrun)
                if placed and any(row[ZIGZAG[z]] for z in range(k, se + 1)):
                    met["history_after_last_new"] = True
                break
            else:
                met["zrl_in_refinement"] = True
            # skip r zero-history coefficients, a correction bit for every non-zero one on the way; stop AT the next zero one
            p0 = bits.p
            while True:
                if k > se:
                    _fail(INVALID, "a run past Se")
                z = ZIGZAG[k]
                if row[z]:
                    if s == 0:
                        met["zrl_over_history"] = True
                        met["zrl_history_between"] = max(met["zrl_history_between"], bits.p - p0 + 1)
                    correct(z)
                else:
                    r -= 1
                    if r < 0:
                        break
                k += 1
            field(bits.p - p0)
            if bits.p - p0:
                met["correction_field_bits_before_new" if s else "correction_field_bits_before_zrl"].add(bits.p - p0)
            if s:
                row[ZIGZAG[k]] = value
                placed = True
                if k == se:
                    met["new_at_se_in_refinement"] = True
            k += 1
    if eobrun > 0:
        p0 = bits.p
        while k <= se:
            if row[ZIGZAG[k]]:
                correct(ZIGZAG[k])
            k += 1
        field(bits.p - p0)
        if entered_in_run and bits.p - p0:
            met["correction_field_bits_in_eob_run"].add(bits.p - p0)
        if entered_in_run and bits.p > p0:
            met["corrections_in_eob_run"] = True
        eobrun -= 1
    return eobrun


def entropy_decode(h, met=None):
    """-> coefficients [blocks, 64] int16, natural order, DESIGN.md 4.16's block store (MCU by MCU, DC values); fills met."""
    met = {} if met is None else met
    met.update({"scans": [], "longest_eob_run": 0, "zrl_in_refinement": False, "zrl_over_history": False, "new_at_se_in_refinement": False,
                "history_after_last_new": False, "corrections_in_eob_run": False, "eob_run_ends_scan": False, "subsequences": [],
                "intervals": 0, "longest_code": 0,
                # the seams of DESIGN.md 4.22's units.  Sets of widths of the fields correct_wave reads at once (all; in front of a new
                # coefficient; in front of a ZRL's target; by a block entered inside an EOB run); a correction bit 1 on a set bit
                "correction_field_bits": set(), "correction_field_bits_before_new": set(), "correction_field_bits_before_zrl": set(),
                "correction_field_bits_in_eob_run": set(), "correction_on_set_bit": 0, "zrl_history_between": 0,
                # (slot, blocks of the scan MCU) at which a subsequence behind an interval's first begins in an interleaved DC-first scan
                "dc_entry_slots": set(),
                # per scan (0 where it is not an AC-first scan): EOBn, n >= 1, whose last bit is the last in front of a subsequence
                # boundary inside its interval; symbols with their value bits, and EOBn with their run bits, on both sides of one
                "eob_run_ends_subsequence": [], "symbol_straddles_subsequence": [], "eobn_straddles_subsequence": [],
                # the byte lengths of the intervals of the file's last AC-refinement scan; the AC-refinement intervals whose last
                # correction bit is the last bit of their last byte (no pad bit)
                "refine_interval_bytes": set(), "refine_interval_without_pad": 0})
    n_blocks = h["mcus_x"] * h["mcus_y"] * h["bpm"]
    coef = [[0] * 64 for _ in range(n_blocks)]
    data = h["data"]
    for scan in h["scans"]:
        ss, se, ah, al = scan["ss"], scan["se"], scan["ah"], scan["al"]
        comps = scan["comps"]
        ri = scan["restart"] or scan["mcus"]
        met["scans"].append((tuple(comps), ss, se, ah, al, scan["restart"], scan["intervals"]))
        dc_lut = {c: t["lut"].tolist() for c, t in scan["dc"].items()}
        ac_lut = scan["ac"]["lut"].tolist() if scan["ac"] else None
        subs = 0
        parts = intervals(data, scan)
        met["intervals"] += len(parts)
        seams = {"eob_run_ends_subsequence": 0, "symbol_straddles_subsequence": 0, "eobn_straddles_subsequence": 0}
        if ss > 0 and ah:
            met["refine_interval_bytes"] = {len(seg) for seg, _ in parts}
        per_mcu = len(mcu_blocks(h, comps, 0, scan["across"]))
        for j, (seg, _where) in enumerate(parts):
            subs += max(1, -(-8 * len(seg) // SUBSEQ_BITS))
            bits = _Bits(seg, met)
            pred = {c: 0 for c in comps}
            eobrun = 0
            last_in_run = False
            boundary = SUBSEQ_BITS   # the first bit of the interval's next subsequence

            def crosses(p0, p1):   # bits p0 .. p1 - 1 lie on both sides of a subsequence boundary of the interval
                return p0 // SUBSEQ_BITS != (p1 - 1) // SUBSEQ_BITS

            for m in range(j * ri, min((j + 1) * ri, scan["mcus"])):
                for slot, (c, idx) in enumerate(mcu_blocks(h, comps, m, scan["across"])):
                    row = coef[idx]
                    if ss == 0 and ah == 0 and len(comps) > 1 and boundary <= bits.p < bits.nbits:
                        met["dc_entry_slots"].add((slot, per_mcu))   # the lane of this subsequence starts at this block
                        boundary = (bits.p // SUBSEQ_BITS + 1) * SUBSEQ_BITS
                    if ss == 0 and ah == 0:
                        s = bits.symbol(dc_lut[c])
                        pred[c] += _extend(bits.get(s), s)
                        row[0] = _wrap16(pred[c] << al)
                    elif ss == 0:
                        if bits.get(1):
                            row[0] = _wrap16(row[0] | 1 << al)
                    elif ah == 0:
                        last_in_run = eobrun > 0
                        if eobrun > 0:
                            eobrun -= 1
                        else:
                            k = ss
                            while k <= se:
                                p0 = bits.p
                                sym = bits.symbol(ac_lut)
                                r, s = sym >> 4, sym & 15
                                if s:
                                    k += r
                                    if k > se:
                                        _fail(INVALID, "a run past Se")
                                    row[ZIGZAG[k]] = _wrap16(_extend(bits.get(s), s) * (1 << al))
                                    seams["symbol_straddles_subsequence"] += crosses(p0, bits.p)
                                    k += 1
                                elif r == 15:
                                    if k + 16 > se + 1:
                                        _fail(INVALID, "a run past Se")
                                    k += 16
                                else:
                                    eobrun = (1 << r) + bits.get(r)
                                    met["longest_eob_run"] = max(met["longest_eob_run"], eobrun)
                                    if r:
                                        seams["eobn_straddles_subsequence"] += crosses(p0, bits.p)
                                        seams["eob_run_ends_subsequence"] += bits.p % SUBSEQ_BITS == 0 and bits.p < bits.nbits
                                    eobrun -= 1
                                    break
                    else:
                        last_in_run = eobrun > 0
                        eobrun = _refine_block(bits, row, ss, se, al, ac_lut, eobrun, met)
                    if bits.p > bits.nbits:
                        _fail(INVALID, "the data ends before the scan's last block")
            if ss > 0 and j + 1 == len(parts) and last_in_run and eobrun == 0:
                met["eob_run_ends_scan"] = True
            if ss > 0 and ah and bits.nbits and bits.p == bits.nbits == bits.last_correction:
                met["refine_interval_without_pad"] += 1
        met["subsequences"].append(subs)
        for key, n in seams.items():
            met[key].append(int(n))
    return np.array(coef, dtype=np.int64).astype(np.int16), met


def pixels_of(h, coef, mode=RGB8, drop_rows=0):
    """The block store -> the pixels, by DESIGN.md 4.16's path (ref_jpeg.decode behind its entropy decode)."""
    w, hh = h["width"], h["height"]
    view = {"comps": [{"h": c["h"], "v": c["v"], "tq": k} for k, c in enumerate(h["comps"])], "quant": {k: c["quant"] for k, c in enumerate(h["comps"])},
            "mcus_x": h["mcus_x"], "mcus_y": h["mcus_y"]}
    pl = ref_jpeg.planes(view, coef)
    if len(pl) == 1:
        y = pl[0][:hh, :w]
        out = y if mode == LUMA8 else np.repeat(y[:, :, None], 3, axis=2)
        return np.ascontiguousarray(out[:hh - drop_rows])
    hs, vs = h["hmax"], h["vmax"]
    y = pl[0][:hh, :w].astype(np.int64)
    dw, dh = -(-w // hs), -(-hh // vs)
    cb, cr = (ref_jpeg.upsample(p, dw, dh, hs, vs)[:hh, :w] - 128 for p in pl[1:])
    r = np.clip(y + ((91881 * cr + 32768) >> 16), 0, 255)
    b = np.clip(y + ((116130 * cb + 32768) >> 16), 0, 255)
    g = np.clip(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255)
    rgb = np.stack([r, g, b], axis=2).astype(np.uint8)
    out = ref_jpeg.luma_of_rgb(rgb) if mode == LUMA8 else rgb
    return np.ascontiguousarray(out[:hh - drop_rows])


def decode(data, mode=RGB8, drop_rows=0, met=None):
    """The file -> [H - drop_rows, W] (LUMA8) or [H - drop_rows, W, 3] (RGB8) uint8."""
    h = parse(data)
    if drop_rows >= h["height"]:
        _fail(INVALID, "drop_rows >= H")
    coef, _ = entropy_decode(h, met)
    return pixels_of(h, coef, mode, drop_rows)
