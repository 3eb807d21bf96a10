"""GPU (-m gpu): every code builder on the synthesised histograms of tests/hist_families.py, table for table against the
oracle.  A wrong sift in a tie does not crash and does not produce an undecodable stream -- it produces a valid prefix
code that merely is not the reference's -- so whole tables are compared, in all five places the wave-parallel heap of
csrc/ghf_build_code.h runs: k_build_code<LIMIT>, k_build_codes<LIMIT>, k_crs_build_code, wave 0 of k_compress_batch and
(under GHF_CODE_LIMIT) the in-kernel package-merge behind it.  Every output is poisoned with 0xA5 before the call and has
guard bytes behind it.  The oracle itself is held to the compiled reference and to plain integer references on the same
histograms by tests/test_hist_families_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import hist_families as hf
import pkgload
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_I32 = int(np.array([POISON] * 4, dtype=np.uint8).view(np.int32)[0])
POISON_U32 = int(np.array([POISON] * 4, dtype=np.uint8).view(np.uint32)[0])
GUARD = 64
E_INVAL, E_EMPTY, E_CODELEN, E_SINGLE = 1, 3, 4, 9
FAMILIES = ("ties", "near", "chain", "wide", "deep")


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


class Arena:
    """outputs of the given sizes in ONE device buffer, each followed by at least GUARD guard bytes; everything 0xA5"""

    def __init__(self, torch, sizes):
        self.sizes, self.at, at = list(sizes), [], 0
        for s in self.sizes:
            self.at.append(at)
            at += (s + GUARD + 63) // 64 * 64
        self.buf = torch.full((max(at, 64),), POISON, dtype=torch.uint8, device="cuda")
        self.end = at
        self.host = None

    def dev(self, i):
        return self.buf[self.at[i] : self.at[i] + self.sizes[i]]

    def fetch(self):
        self.host = self.buf.cpu().numpy()

    def payload(self, i, part=0, part_bytes=None):
        n = self.sizes[i] if part_bytes is None else part_bytes
        return self.host[self.at[i] + part * n : self.at[i] + (part + 1) * n].tobytes()

    def guards_intact(self):
        ends = self.at[1:] + [self.end]
        return all((self.host[a + s : e] == POISON).all() for a, s, e in zip(self.at, self.sizes, ends))


def sync_status(ghf, ctx):
    """the status the queued work latched (0: none); the context is usable again afterwards"""
    try:
        ctx.sync()
    except ghf.GhfError as e:
        return e.status
    return 0


class World:
    """the family on the device, and the oracle's answers, computed once"""

    def __init__(self, ghf, ctx, torch):
        self.fam = hf.family()
        self.code_bytes = C.sizeof(ghf.Code)
        self.tree_bytes = C.sizeof(ghf.Tree)
        self.d_hists = torch.from_numpy(np.stack([h for _, h, _ in self.fam])).cuda()  # int64[N, 257] (uint64 bit patterns)
        self.fits = [i for i, (_, _, k) in enumerate(self.fam) if k == "fits"]
        self.deep = [i for i, (_, _, k) in enumerate(self.fam) if k == "deep"]
        self.ood = [i for i, (_, _, k) in enumerate(self.fam) if k == "out_of_domain"]
        self.want = {i: orc.build_code(self.fam[i][1]).as_dict() for i in self.fits}
        self.want_limited = {i: orc.build_code_limited(self.fam[i][1], 32).as_dict() for i in self.deep}
        # ghf_build_code on every `fits` entry, in family order (large and small heaps alternate), one sync
        arena = Arena(torch, [self.code_bytes] * len(self.fits))
        for j, i in enumerate(self.fits):
            ctx.build_code(self.d_hists[i], arena.dev(j))
        self.single_status = sync_status(ghf, ctx)
        arena.fetch()
        self.single_guards = arena.guards_intact()
        self.single = {i: arena.payload(j) for j, i in enumerate(self.fits)}

    def family_of(self, i):
        return self.fam[i][0].split("/")[0]


@pytest.fixture(scope="module")
def world(env):
    return World(*env)


def code_dict(ghf, raw):
    return ghf.Code.from_buffer_copy(raw).as_dict()


def unfinished(ghf, raw):
    c = ghf.Code.from_buffer_copy(raw)
    return c.max_len == POISON_I32 and c.min_len == POISON_I32


# ---------------------------------------------------------------------------------------------- ghf_build_code
@pytest.mark.parametrize("family", FAMILIES)
def test_build_code_equals_the_oracle(env, world, family):
    ghf, ctx, torch = env
    assert world.single_status == 0 and world.single_guards
    mine = [i for i in world.fits if world.family_of(i) == family]
    assert mine
    for i in mine:
        assert code_dict(ghf, world.single[i]) == world.want[i], world.fam[i][0]


def test_build_code_refuses_deep_entries_and_goes_on(env, world):
    ghf, ctx, torch = env
    assert len(world.deep) >= 13
    arena = Arena(torch, [world.code_bytes] * (2 * len(world.deep)))
    for j, i in enumerate(world.deep):
        ctx.build_code(world.d_hists[i], arena.dev(2 * j))
        assert sync_status(ghf, ctx) == E_CODELEN, world.fam[i][0]
        ctx.build_code(world.d_hists[world.fits[j]], arena.dev(2 * j + 1))  # the context builds a code that fits right after
        assert sync_status(ghf, ctx) == 0
    arena.fetch()
    assert arena.guards_intact()
    for j, i in enumerate(world.deep):
        assert unfinished(ghf, arena.payload(2 * j)), world.fam[i][0]
        assert code_dict(ghf, arena.payload(2 * j + 1)) == world.want[world.fits[j]]


# ---------------------------------------------------------------------------------------------- ghf_build_code_ex
@pytest.mark.parametrize("family", FAMILIES)
def test_code_limit_changes_nothing_where_the_code_fits(env, world, family):
    ghf, ctx, torch = env
    mine = [i for i in world.fits if world.family_of(i) == family]
    arena = Arena(torch, [world.code_bytes] * len(mine))
    for j, i in enumerate(mine):
        ctx.build_code(world.d_hists[i], arena.dev(j), flags=ghf.CODE_LIMIT)
    assert sync_status(ghf, ctx) == 0
    arena.fetch()
    assert arena.guards_intact()
    for j, i in enumerate(mine):
        assert arena.payload(j) == world.single[i], world.fam[i][0]
        assert code_dict(ghf, arena.payload(j)) == world.want[i], world.fam[i][0]


def test_code_limit_on_deep_entries_equals_the_oracle_package_merge(env, world):
    """PARITY UNPINNED (the reference has no such code): the oracle's definition, itself held to an integer package-merge"""
    ghf, ctx, torch = env
    arena = Arena(torch, [world.code_bytes] * len(world.deep))
    for j, i in enumerate(world.deep):
        ctx.build_code(world.d_hists[i], arena.dev(j), flags=ghf.CODE_LIMIT)
    assert sync_status(ghf, ctx) == 0
    arena.fetch()
    assert arena.guards_intact()
    for j, i in enumerate(world.deep):
        assert world.want_limited[i]["max_len"] == 32
        assert code_dict(ghf, arena.payload(j)) == world.want_limited[i], world.fam[i][0]


def test_code_limit_with_empty_ok_on_the_lone_end_mark(env, world):
    ghf, ctx, torch = env
    h = np.zeros(257, dtype=np.int64)
    h[256] = 1
    arena = Arena(torch, [world.code_bytes])
    ctx.build_code(torch.from_numpy(h).cuda(), arena.dev(0), flags=ghf.CODE_LIMIT | ghf.EMPTY_OK)
    assert sync_status(ghf, ctx) == 0
    arena.fetch()
    assert arena.guards_intact()
    want = orc.OrcCode()  # the table behind orc.compress_empty(), which tests/test_gpu_limit.py expects as a stream
    for s in range(257):
        want.symbol[s] = 0xFFFFFFFF
    want.symbol[0] = 256
    want.length[256] = 1
    want.min_len = want.max_len = 1
    assert code_dict(ghf, arena.payload(0)) == want.as_dict()


# ---------------------------------------------------------------------------------------------- ghf_build_codes
def test_build_codes_in_launches_of_one_to_eight(env, world):
    ghf, ctx, torch = env
    d_fits = world.d_hists[torch.tensor(world.fits, device="cuda")].contiguous()  # the `fits` rows, in order
    launches, at, turn = [], 0, 0
    while at < len(world.fits):
        n = min(1 + turn % 8, len(world.fits) - at)
        launches.append((at, n, ghf.CODE_LIMIT if (turn // 8) & 1 else 0))
        at += n
        turn += 1
    assert {n for _, n, _ in launches} == set(range(1, 9))
    assert {(n, f) for _, n, f in launches} >= {(n, f) for n in range(1, 9) for f in (0, ghf.CODE_LIMIT)}
    arena = Arena(torch, [n * world.code_bytes for _, n, _ in launches])
    for k, (a, n, flags) in enumerate(launches):
        ctx.build_codes(d_fits[a : a + n], arena.dev(k), flags=flags)
    assert sync_status(ghf, ctx) == 0
    arena.fetch()
    assert arena.guards_intact()
    for k, (a, n, flags) in enumerate(launches):
        for p in range(n):
            i = world.fits[a + p]
            raw = arena.payload(k, p, world.code_bytes)
            assert raw == world.single[i], (world.fam[i][0], n, p, flags)
            assert code_dict(ghf, raw) == world.want[i], (world.fam[i][0], n, p, flags)


def launch_of_eight(env, world, odd_one, slot, flags, salt):
    """one ghf_build_codes launch of eight: seven `fits` entries and `odd_one` in `slot` -> (status, [raw code] * 8, members)"""
    ghf, ctx, torch = env
    good = [world.fits[(37 * salt + 101 * slot + 13 * q) % len(world.fits)] for q in range(7)]
    members = good[:slot] + [odd_one] + good[slot:]
    d_h = world.d_hists[torch.tensor(members, device="cuda")].contiguous()
    arena = Arena(torch, [8 * world.code_bytes])
    ctx.build_codes(d_h, arena.dev(0), flags=flags)
    status = sync_status(ghf, ctx)
    arena.fetch()
    assert arena.guards_intact()
    return status, [arena.payload(0, p, world.code_bytes) for p in range(8)], members


@pytest.mark.parametrize("slot", range(8))
def test_build_codes_with_one_deep_member(env, world, slot):
    ghf, ctx, torch = env
    deep = world.deep[slot]
    status, raws, members = launch_of_eight(env, world, deep, slot, 0, 1)
    assert status == E_CODELEN
    for p, i in enumerate(members):
        if p == slot:
            assert unfinished(ghf, raws[p])
        else:
            assert code_dict(ghf, raws[p]) == world.want[i], (world.fam[i][0], p)
    status, raws, members = launch_of_eight(env, world, deep, slot, ghf.CODE_LIMIT, 2)
    assert status == 0
    for p, i in enumerate(members):
        assert code_dict(ghf, raws[p]) == (world.want_limited[i] if p == slot else world.want[i]), (world.fam[i][0], p)


# ---------------------------------------------------------------------------------------------- ghf_crs_build_code
def walk_tree(tree):
    """Tree.code_strings() with a budget: a wrong tree must fail the test, not hang it"""
    out, stack, visited = [""] * 256, [(tree.root, "")], 0
    while stack:
        node, path = stack.pop()
        visited += 1
        assert visited <= 511 and node < 512, "not a tree"
        if node < 256:
            out[node] = path
        else:
            stack.append((tree.right[node - 256], path + "1"))
            stack.append((tree.left[node - 256], path + "0"))
    return out


def crs_expectation(h256):
    """-> (status, oracle tree or None, its code strings or None) for the 256 counts (uint64 bit patterns)"""
    live = int(np.count_nonzero(h256))
    if sum(int(x) for x in h256.view(np.uint64)) >= 1 << 55:
        return E_INVAL, None, None
    if live < 2:
        return (E_EMPTY if live == 0 else E_SINGLE), None, None
    t = orc.crs_tree(h256)
    codes = orc.crs_code_strings(t)
    return (E_CODELEN if max(len(c) for c in codes) > 64 else 0), t, codes


def check_crs(ghf, label, raw_tree, raw_code, t, codes):
    tree = ghf.Tree.from_buffer_copy(raw_tree)
    header = orc.crs_tree_bytes(t)
    depth = max(len(c) for c in codes)
    assert (tree.tree_bytes, tree.n_leaves, tree.max_len) == (header.size, t.n_leaves, depth), label
    assert bytes(tree.header[: tree.tree_bytes]) == header.tobytes(), label
    assert walk_tree(tree) == codes, label
    code = ghf.Code.from_buffer_copy(raw_code)
    assert (code.min_len, code.max_len) == (min(len(c) for c in codes if c), depth), label
    assert code.length[256] == 0 and code.codeword[256] == 0, label
    for s, cs in enumerate(codes):
        # above depth 32, bits 32..63 of a code sit in symbol[] (include/ghf.h, ghf_crs_build_code)
        full = code.codeword[s] | ((code.symbol[s] << 32) if depth > 32 else 0)
        assert code.length[s] == len(cs) and full == (int(cs, 2) if cs else 0), (label, s)
        if depth <= 32:
            assert code.symbol[s] == 0xFFFFFFFF, (label, s)


def run_crs(env, world, entries):
    """entries: [(label, int64[256])].  The accepted ones go out back to back with one sync, the refused ones one by one."""
    ghf, ctx, torch = env
    expect = [crs_expectation(h) for _, h in entries]
    d_h = torch.from_numpy(np.stack([h for _, h in entries])).cuda()  # int64[N, 256]: no slot [256] to read
    arena = Arena(torch, [world.tree_bytes, world.code_bytes] * len(entries))
    for j, (status, _, _) in enumerate(expect):
        if status == 0:
            ctx.crs_build_code(d_h[j], arena.dev(2 * j), arena.dev(2 * j + 1))
    assert sync_status(ghf, ctx) == 0
    for j, (status, _, _) in enumerate(expect):
        if status != 0:
            ctx.crs_build_code(d_h[j], arena.dev(2 * j), arena.dev(2 * j + 1))
            assert sync_status(ghf, ctx) == status, entries[j][0]
    arena.fetch()
    assert arena.guards_intact()
    for j, (status, t, codes) in enumerate(expect):
        if status == 0:
            check_crs(ghf, entries[j][0], arena.payload(2 * j), arena.payload(2 * j + 1), t, codes)
        else:  # no finished tree, no finished code
            assert ghf.Tree.from_buffer_copy(arena.payload(2 * j)).max_len == POISON_U32, entries[j][0]
            assert unfinished(ghf, arena.payload(2 * j + 1)), entries[j][0]
    return [status for status, _, _ in expect]


@pytest.mark.parametrize("family", FAMILIES)
def test_crs_build_code_equals_the_oracle(env, world, family):
    entries = [(label, h[:256]) for label, h, _ in world.fam if label.split("/")[0] == family and hf.n_live(h) >= 2]
    statuses = run_crs(env, world, entries)
    refused = [entries[j][0] for j, s in enumerate(statuses) if s != 0]
    assert refused == (["deep/fib75"] if family == "deep" else [])  # depth 74: beyond the 64 bits a .crs code may have


def test_crs_build_code_at_depth_63_64_65_and_without_a_tree(env, world):
    extras = hf.crs_extras()
    statuses = run_crs(env, world, [(label, h) for label, h, _ in extras])
    assert statuses == [0, 0, E_CODELEN, E_EMPTY, E_SINGLE]
    assert [e for _, _, e in extras] == [63, 64, 65, "empty", "single"]


# ---------------------------------------------------------------------------------------------- k_compress_batch
@pytest.mark.parametrize("part", range(3))
def test_compress_batch_builds_the_oracle_tables(env, world, part):
    """wave 0 of k_compress_batch: build_code_body with code_sync<false>, counts from the workgroup's LDS bins"""
    ghf, ctx, torch = env
    pinned = hf.pinned()
    mine = pinned[part::3]
    assert len(pinned) >= 600 and mine
    datas = [hf.materialise(i, h) for i, _, h in mine]
    packed = torch.from_numpy(np.concatenate(datas)).cuda()
    d_codes = torch.full((len(mine) + 1, world.code_bytes), POISON, dtype=torch.uint8, device="cuda")  # last row: guard
    r = ctx.compress_batch(packed, sizes=[d.size for d in datas], max_item_bytes=hf.PIN_TOTAL, d_codes=d_codes)
    assert sync_status(ghf, ctx) == 0
    assert not r["status"].any().item()
    h_codes, h_out, h_nb = d_codes.cpu().numpy(), r["out"].cpu().numpy(), r["out_bytes"].cpu().numpy()
    assert (h_codes[len(mine)] == POISON).all()
    for j, (i, label, h) in enumerate(mine):
        assert code_dict(ghf, h_codes[j].tobytes()) == world.want[i], label
        ref = orc.compress(datas[j])
        assert h_nb[j] == ref.size and np.array_equal(h_out[j * r["out_stride"] :][: ref.size], ref), label


# ---------------------------------------------------------------------------------------------- the counts' domain
def by_label(world, label):
    return next(i for i, (l, _, _) in enumerate(world.fam) if l == label)


def test_the_last_totals_inside_the_domain(env, world):
    ghf, ctx, torch = env
    for label in ("wide/total-2^55-555", "wide/total-2^55-1"):
        i = by_label(world, label)
        assert hf.total(world.fam[i][1]) in ((1 << 55) - 555, (1 << 55) - 1)
        assert code_dict(ghf, world.single[i]) == world.want[i], label
        for flags in (0, ghf.CODE_LIMIT):
            status, raws, members = launch_of_eight(env, world, i, 5, flags, 3)
            assert status == 0
            assert [code_dict(ghf, raw) for raw in raws] == [world.want[m] for m in members], (label, flags)
        assert run_crs(env, world, [(label, world.fam[i][1][:256])]) == [0]


def test_counts_out_of_the_domain_are_refused(env, world):
    """2^55 and more in the 257 counts: a node's weight no longer fits the heap word beside the 9-bit index (include/ghf.h,
    ghf_build_code).  GHF_E_INVAL, and nothing that looks like a finished code."""
    ghf, ctx, torch = env
    assert {world.fam[i][0] for i in world.ood} == {"ood/total-2^55", "ood/two-2^54", "ood/single-2^55", "ood/single-2^63",
                                                    "ood/single-2^64-1"}
    for slot, i in enumerate(world.ood):
        label = world.fam[i][0]
        assert hf.total(world.fam[i][1]) >= 1 << 55
        for flags in (0, ghf.CODE_LIMIT):
            arena = Arena(torch, [world.code_bytes])
            ctx.build_code(world.d_hists[i], arena.dev(0), flags=flags)
            assert sync_status(ghf, ctx) == E_INVAL, (label, flags)
            arena.fetch()
            assert arena.guards_intact() and unfinished(ghf, arena.payload(0)), (label, flags)
            # ghf_build_codes: refused among good neighbours, which are built all the same
            status, raws, members = launch_of_eight(env, world, i, slot, flags, 4)
            assert status == E_INVAL, (label, flags)
            for p, m in enumerate(members):
                if p == slot:
                    assert unfinished(ghf, raws[p]), (label, flags)
                else:
                    assert code_dict(ghf, raws[p]) == world.want[m], (label, flags, p)
    # ghf_crs_build_code reads the 256 byte counts alone: "ood/total-2^55" is 2^55 - 1 there, inside the domain, and must
    # equal the oracle; "ood/two-2^54" is the same edge for it
    statuses = run_crs(env, world, [(world.fam[i][0], world.fam[i][1][:256]) for i in world.ood])
    assert statuses == [0 if world.fam[i][0] == "ood/total-2^55" else E_INVAL for i in world.ood]
    # the context still builds
    arena = Arena(torch, [world.code_bytes])
    ctx.build_code(world.d_hists[world.fits[0]], arena.dev(0))
    assert sync_status(ghf, ctx) == 0
    arena.fetch()
    assert code_dict(ghf, arena.payload(0)) == world.want[world.fits[0]]
