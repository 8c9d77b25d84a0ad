"""LDS bank-conflict model of the register-chained W&D kernel's access patterns (csrc/wd_chain.hip).

Per-instruction lane groups and bank functions from MI355X_MICROARCH.md §LDS: a wave-instruction is serviced
in fixed lane groups, one LDS cycle per group when conflict-free; within a group each extra distinct dword
address on a bank adds a cycle. `python tools/lds_banks.py` prints cycles per instruction (ideal = number of
groups) for every access site under the current layout and candidate swizzles."""
from __future__ import annotations

import itertools
from collections import defaultdict

GROUPS = {
    "b64": [list(range(32)), list(range(32, 64))],  # ds_read_b64 / ds_read_b64_tr_b16
    "b128": [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)],
             [*range(32, 36), *range(44, 48), *range(52, 60)], [*range(36, 44), *range(48, 52), *range(60, 64)]],
    "w64": [list(range(16 * i, 16 * i + 16)) for i in range(4)],  # ds_write_b64
    "w128": [list(range(8 * i, 8 * i + 8)) for i in range(8)],  # ds_write_b128
}
NBANK = {"b64": 64, "b128": 64, "w64": 32, "w128": 32}
WIDTH = {"b64": 8, "b128": 16, "w64": 8, "w128": 16}


def cycles(addrs: list[int], kind: str) -> int:
    """addrs: byte address per lane (64); returns LDS cycles of the wave-instruction."""
    tot = 0
    for g in GROUPS[kind]:
        banks = defaultdict(set)
        for lane in g:
            for d in range(WIDTH[kind] // 4):
                dw = addrs[lane] // 4 + d
                banks[dw % NBANK[kind]].add(dw)
        tot += max(len(v) for v in banks.values())
    return tot


class Layout:
    """row-major bf16 image [rows][cols + pad] with an optional XOR swizzle of 8-byte (4-element) granules
    (gran: 4-element granule index within the row) by a function of the row."""

    def __init__(self, cols: int, pad: int = 8, swz=None):
        self.cols, self.pad, self.swz = cols, pad, swz

    def addr(self, row: int, col: int) -> int:
        g, e = divmod(col, 4)
        if self.swz is not None:
            g = self.swz(row, g, self.cols // 4)
        return 2 * (row * (self.cols + self.pad) + 4 * g + e)


def lane_rh(lane):
    return lane & 15, lane >> 4


def fwd_read(L: Layout, K, N):
    """ld8: lane (r, h) reads row 16 nt + r, elements 32 s + 8 h .. +7 (ds_read_b128)."""
    out = []
    for nt in range(N // 16):
        for s in range(K // 32):
            a = [L.addr(16 * nt + (l & 15), 32 * s + 8 * (l >> 4)) for l in range(64)]
            out.append(cycles(a, "b128"))
    return out


def dA_read(L: Layout, K, N):
    """tr_read: lane 4q+p of group h supplies row 32 s + 16(h%2) + 4(h/2) + q (+8), cols 16 kt + 4 p."""
    out = []
    for s in range(N // 32):
        for kt in range(K // 16):
            for second in (0, 8):
                a = []
                for l in range(64):
                    r, h = lane_rh(l)
                    q, p = r >> 2, r & 3
                    a.append(L.addr(32 * s + 16 * (h & 1) + 4 * (h >> 1) + q + second, 16 * kt + 4 * p))
                out.append(cycles(a, "b64"))
    return out


def dw_read(L: Layout, cols):
    """dw_phase tr_read of a staged [T][cols] image: row 32 ts + 8 h + q (+4), cols 16 t + 4 p."""
    out = []
    for ts in range(4):
        for t in range(cols // 16):
            for second in (0, 4):
                a = []
                for l in range(64):
                    r, h = lane_rh(l)
                    q, p = r >> 2, r & 3
                    a.append(L.addr(32 * ts + 8 * h + q + second, 16 * t + 4 * p))
                out.append(cycles(a, "b64"))
    return out


def stage_writes(LZ: Layout, LA: Layout, K, N, epw=16):
    """dZ: ds_write_b64 at row (epw w + 16 tb + r), natural col f0(kt, h); A: ds_write_b128 at col 32 s + 8 h."""
    outz, outa = [], []
    w = 0
    for kt in range(N // 16):
        a = []
        for l in range(64):
            r, h = lane_rh(l)
            f0 = 32 * (kt >> 1) + 16 * (h & 1) + 8 * (kt & 1) + 4 * (h >> 1)
            a.append(LZ.addr(epw * w + r, f0))
        outz.append(cycles(a, "w64"))
    for s in range(K // 32):
        a = [LA.addr(epw * w + (l & 15), 32 * s + 8 * (l >> 4)) for l in range(64)]
        outa.append(cycles(a, "w128"))
    return outz, outa


def mask_read(LA: Layout, K, epw=16):
    out = []
    for kt in range(K // 16):
        a = [LA.addr(epw * 0 + (l & 15), 16 * kt + 4 * (l >> 4)) for l in range(64)]
        out.append(cycles(a, "b64"))
    return out


LAYERS = [(32, 128), (128, 96), (96, 64), (64, 64), (64, 16)]


def report(name, wl, sl):
    """wl(K) -> weight layout for a W^T image with K columns; sl(cols) -> staging layout."""
    tot = defaultdict(lambda: [0, 0])
    for li, (K, N) in enumerate(LAYERS):
        f = fwd_read(wl(K), K, N)
        tot["fwd b128"][0] += sum(f)
        tot["fwd b128"][1] += 4 * len(f)
        if li > 0 and N >= 32:
            d = dA_read(wl(K), K, N)
            tot["dA tr"][0] += sum(d)
            tot["dA tr"][1] += 2 * len(d)
        for cols in (N, K):
            if cols >= 16:
                d = dw_read(sl(cols), cols)
                tot["dW tr"][0] += sum(d)
                tot["dW tr"][1] += 2 * len(d)
        if N >= 32:
            z, a = stage_writes(sl(N), sl(K), K, N)
            tot["stage dZ w64"][0] += sum(z)
            tot["stage dZ w64"][1] += 4 * len(z)
            tot["stage A w128"][0] += sum(a)
            tot["stage A w128"][1] += 8 * len(a)
        m = mask_read(sl(K), K)
        tot["mask b64"][0] += sum(m)
        tot["mask b64"][1] += 2 * len(m)
    print(f"== {name}")
    for k, (c, ideal) in tot.items():
        print(f"   {k:>14}: {c:6d} cycles (ideal {ideal:6d}, x{c / ideal:.2f})")


def main():
    report("current: pad 8 everywhere", lambda K: Layout(K, 8), lambda c: Layout(c, 8))
    for pw, ps in itertools.product((0, 4, 8, 16), (0, 4, 8, 16)):
        report(f"pad weights {pw}, staging {ps}", lambda K, pw=pw: Layout(K, pw), lambda c, ps=ps: Layout(c, ps))


if __name__ == "__main__" and __import__("sys").argv[1:] != ["opt"]:
    main()


def xor_swz(masks):
    """granule g of row -> g ^ (XOR of masks[b] over the set bits b of row)."""
    def f(row, g, ngran):
        m = 0
        for b, mb in enumerate(masks):
            if (row >> b) & 1:
                m ^= mb
        return g ^ m
    return f


def staging_cost(L: Layout, cols: int, as_dz: bool, as_a: bool, K_for_mask: bool) -> int:
    c = sum(dw_read(L, cols))
    if as_dz:
        c += sum(stage_writes(L, Layout(16, 8), 32, cols)[0]) if cols >= 32 else 0
    if as_a:
        c += sum(stage_writes(Layout(32, 8), L, cols, 32)[1]) if cols >= 32 else 0
        c += sum(mask_read(L, cols))
    return c


def weight_cost(L: Layout, K: int, N: int) -> int:
    c = sum(fwd_read(L, K, N))
    if N >= 32:
        c += sum(dA_read(L, K, N))
    return c


def search(cost, cols, pads=(0, 8, 16), passes=2):
    """coordinate descent over pad and per-row-bit XOR masks (even, within the largest power-of-two block
    that divides the granule count) -> (cost, pad, masks)"""
    ngran = cols // 4
    blk = 1
    while ngran % (blk * 2) == 0 and blk * 2 <= 32:
        blk *= 2
    best = None
    for pad in pads:
        masks = [0] * 7
        cur = cost(Layout(cols, pad))
        for _ in range(passes):
            for b in range(7):
                for m in range(0, blk, 2):
                    trial = masks[:b] + [m] + masks[b + 1:]
                    c = cost(Layout(cols, pad, xor_swz(trial) if any(trial) else None))
                    if c < cur:
                        cur, masks = c, trial
        if best is None or cur < best[0]:
            best = (cur, pad, masks)
    return best


def optimise():
    print("== weight images (fwd row reads + dA transposed reads)")
    for K, N in LAYERS:
        ideal = sum(4 for _ in range((N // 16) * (K // 32))) + (2 * 2 * (N // 32) * (K // 16) if N >= 32 else 0)
        cur = weight_cost(Layout(K, 8), K, N)
        best = search(lambda L, K=K, N=N: weight_cost(L, K, N), K)
        print(f"   K={K:3d} N={N:3d}: current {cur}, best {best[0]} (ideal {ideal}) pad {best[1]} masks {best[2]}")
    print("== staging images (dW transposed reads + writes + mask reads)")
    for cols, dz, a in ((16, True, False), (64, True, True), (96, True, True), (128, True, True), (32, False, True)):
        cur = staging_cost(Layout(cols, 8), cols, dz, a, a)
        best = search(lambda L, cols=cols, dz=dz, a=a: staging_cost(L, cols, dz, a, a), cols)
        print(f"   cols={cols:3d} dz={dz} a={a}: current {cur}, best {best[0]} pad {best[1]} masks {best[2]}")


if __name__ == "__main__" and __import__("sys").argv[1:] == ["opt"]:
    optimise()


def rowbit3_swz(mask_gran):
    """XOR the granule index with mask_gran on rows whose bit 3 is set (cheap: bit 3 of the row is lane-dependent
    in every staging access, so at most two address variants per access pattern)."""
    def f(row, g, ngran):
        return g ^ (mask_gran if (row >> 3) & 1 else 0)
    return f


def staging_candidates():
    print("== staging: pad + (row bit 3 -> granule XOR 16) candidates")
    for cols in (64, 96, 128):
        base = staging_cost(Layout(cols, 8), cols, True, True, True)
        res = []
        for pad in (8, 16, 24, 32):
            for m in (0, 16):
                if m >= cols // 4:
                    continue
                L = Layout(cols, pad, rowbit3_swz(m) if m else None)
                res.append((staging_cost(L, cols, True, True, True), pad, m,
                            sum(dw_read(L, cols)), sum(stage_writes(L, L, cols, cols)[0]),
                            sum(stage_writes(L, L, cols, cols)[1]), sum(mask_read(L, cols))))
        res.sort()
        print(f"   cols {cols}: current (pad 8) {base}; best: " + "; ".join(
            f"cost {c} pad {p} xor {m} (dW {a} dZw {b} Aw {c2} mask {d})" for c, p, m, a, b, c2, d in res[:3]))


if __name__ == "__main__" and __import__("sys").argv[1:] == ["stage"]:
    staging_candidates()


class PermLayout(Layout):
    """row-major image with row stride cols + pad and a physical row permutation perm(row)."""

    def __init__(self, cols, pad, perm):
        super().__init__(cols, pad)
        self.perm = perm

    def addr(self, row, col):
        return super().addr(self.perm(row), col)


def wperm(n):
    return n ^ (((n >> 4) & 1) << 2)


def sperm(t):
    return t ^ (((t >> 3) & 1) << 2)


def perm_report():
    print("== row-permuted layouts (weights: pad 16 + rows 16-31 of each 32-block XOR 4; staging: pad 16 + rows "
          "8-15 of each 16-block XOR 4)")
    report("pad 16 / pad 8 (current)", lambda K: Layout(K, 16), lambda c: Layout(c, 8))
    report("permuted", lambda K: PermLayout(K, 16, wperm), lambda c: PermLayout(c, 16, sperm))


if __name__ == "__main__" and __import__("sys").argv[1:] == ["perm"]:
    perm_report()


def sperm2(t):
    """staging row permutation: inside each 16-row block, row bits (b3 b2 b1 b0) -> (b3 b1 b0 b2), so the 8 rows a
    32-lane half of a dW transposed read touches (q, 8+q) land on physical rows of one parity."""
    return (t & ~15) | (t & 8) | ((t & 3) << 1) | ((t >> 2) & 1)


def stage_writes_c(LZ, LA, K, N, epw=16):
    """dZ staged in C order with 16-byte writes (cat of tiles 2m, 2m+1 at C position 32m + 8h)."""
    outz, outa = [], []
    for m in range(N // 32):
        a = [LZ.addr(epw * 0 + (l & 15), 32 * m + 8 * (l >> 4)) for l in range(64)]
        outz.append(cycles(a, "w128"))
    for s in range(K // 32):
        a = [LA.addr(epw * 0 + (l & 15), 32 * s + 8 * (l >> 4)) for l in range(64)]
        outa.append(cycles(a, "w128"))
    return outz, outa


def perm2_report():
    wl = lambda K: PermLayout(K, 16, wperm)  # noqa: E731
    sl = lambda c: PermLayout(c, 8, sperm2)  # noqa: E731
    tot = defaultdict(lambda: [0, 0])
    for li, (K, N) in enumerate(LAYERS):
        f = fwd_read(wl(K), K, N)
        tot["fwd b128"][0] += sum(f)
        tot["fwd b128"][1] += 4 * len(f)
        if li > 0 and N >= 32:
            d = dA_read(wl(K), K, N)
            tot["dA tr"][0] += sum(d)
            tot["dA tr"][1] += 2 * len(d)
        for cols in (N, K):
            if cols >= 16:
                d = dw_read(sl(cols), cols)
                tot["dW tr"][0] += sum(d)
                tot["dW tr"][1] += 2 * len(d)
        if N >= 32:
            z, a = stage_writes_c(sl(N), sl(K), K, N)
            tot["stage dZ w128"][0] += sum(z)
            tot["stage dZ w128"][1] += 8 * len(z)
            tot["stage A w128"][0] += sum(a)
            tot["stage A w128"][1] += 8 * len(a)
        m = mask_read(sl(K), K)
        tot["mask b64"][0] += sum(m)
        tot["mask b64"][1] += 2 * len(m)
    print("== weights pad 16 + wperm; staging pad 8 + sperm2, dZ in C order (16-B writes)")
    for k, (c, ideal) in tot.items():
        print(f"   {k:>14}: {c:6d} cycles (ideal {ideal:6d}, x{c / ideal:.2f})")


if __name__ == "__main__" and __import__("sys").argv[1:] == ["perm2"]:
    perm2_report()


def stage_writes_nat(LZ, LA, K, N, epw=16):
    """dZ staged with natural 16-column tiles: the 16-byte pair of lane group h (C positions 32 m + 8 h) goes to
    column 32 m + 8 (2 (h & 1) + (h >> 1)) -- csrc/wd_chain.hip stage(). A side as stage_writes_c."""
    outz = []
    for m in range(N // 32):
        a = [LZ.addr(epw * 0 + (l & 15), 32 * m + 8 * (2 * ((l >> 4) & 1) + (l >> 5))) for l in range(64)]
        outz.append(cycles(a, "w128"))
    return outz, stage_writes_c(LZ, LA, K, N, epw)[1]


# live tiles per layer (csrc/wd_chain.hip FN / DN / KT): forward n tiles, dW n tiles, C-order k tiles
LIVE = [(7, 7, 1), (5, 5, 7), (4, 3, 5), (3, 3, 4), (1, 1, 3)]


def nat_report():
    """The kernel as built: weights pad 16 + wperm, staging pad 8 + sperm2, dZ staged in natural tiles, and only
    the live tiles read (fwd: FN n tiles; dA: KT k tiles x the k-steps holding a live dZ tile; dW: DN + KT tiles;
    mask: KT tiles). The stage writes full rows."""
    wl = lambda K: PermLayout(K, 16, wperm)  # noqa: E731
    sl = lambda c: PermLayout(c, 8, sperm2)  # noqa: E731
    tot = defaultdict(lambda: [0, 0])

    def add(key, cyc, ideal_each):
        tot[key][0] += sum(cyc)
        tot[key][1] += ideal_each * len(cyc)

    for li, ((K, N), (fn, dn, kt)) in enumerate(zip(LAYERS, LIVE)):
        ks = K // 32
        add("fwd b128", fwd_read(wl(K), K, N)[:fn * ks], 4)
        if li > 0 and N >= 32:
            ns_live = (LIVE[li + 1][2] + 1) // 2  # k-steps of the dA product with a live dZ tile
            d = dA_read(wl(K), K, N)  # ordered s, kt, (first, second)
            kt_all = K // 16
            add("dA tr", [d[(s * kt_all + t) * 2 + i] for s in range(ns_live) for t in range(kt) for i in (0, 1)], 2)
        if N >= 16:
            dz = dw_read(sl(N), N)  # ordered ts, tile, (first, second)
            add("dW tr", [dz[(ts * (N // 16) + t) * 2 + i] for ts in range(4) for t in range(dn) for i in (0, 1)], 2)
        da = dw_read(sl(K), K)
        add("dW tr", [da[(ts * (K // 16) + t) * 2 + i] for ts in range(4) for t in range(kt) for i in (0, 1)], 2)
        if N >= 32:
            z, a = stage_writes_nat(sl(N), sl(K), K, N)
            add("stage dZ w128", z, 8)
            add("stage A w128", a, 8)
        add("mask b64", mask_read(sl(K), K)[:kt], 2)
    print("== weights pad 16 + wperm; staging pad 8 + sperm2, dZ in natural tiles (16-B writes), live tiles only")
    for k, (c, ideal) in tot.items():
        print(f"   {k:>14}: {c:6d} cycles (ideal {ideal:6d}, x{c / ideal:.2f})")


if __name__ == "__main__" and __import__("sys").argv[1:] == ["nat"]:
    nat_report()
