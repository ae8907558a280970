"""Source-level drop-in: the SAME input deck file the reference executable was built from
(oracle/decks/plumbing16.cxx, BASELINE configs[0]) is compiled, unmodified, against the HIP host
(old-vpic_amd/host) and its output files are compared with what the reference executable wrote
(tests/golden/deck16.npz).  GPU box only."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib_env(env=None):
    """The environment for an executable linked against libvpic_hip.so: this tree's library first on the loader's path, so
    that the executable finds it wherever it lies (oracle/_ref/ may have been built in another copy of the tree)."""
    env = dict(os.environ if env is None else env)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(d for d in (os.path.join(ROOT, "old-vpic_amd"), env.get("LD_LIBRARY_PATH")) if d)
    return env


def run_deck(cmd, **kw):
    """subprocess.check_call for a deck executable with its output kept out of the test log -- unless the run fails: then
    the tail of what it wrote is the assertion message."""
    kw.pop("stdout", None); kw.pop("stderr", None)
    kw["env"] = lib_env(kw.get("env"))
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, **kw)
    assert r.returncode == 0, "%s -> exit %d\n%s" % (" ".join(str(c) for c in cmd[:4]), r.returncode, (r.stderr or "")[-3000:])
    return r


@pytest.fixture(autouse=True)
def _ranks_share_the_one_gpu(monkeypatch):
    """The box has ONE GPU: the mpiexec -n 2 / -n 4 runs of this module put several ranks on it, which RCCL -- the deck
    host's default transport between ranks -- refuses.  They ask for the host-staged MPI transport (the same exchange
    choreography, every message through host memory); tests/test_gpu_rccl_host.py runs the RCCL transport on one rank
    that sends to itself."""
    monkeypatch.setenv("VPIC_HIP_HOST_TRANSPORT", "mpi")


def test_reference_deck_runs_on_the_hip_host(tmp_path):
    importlib.import_module("old-vpic_amd").lib()           # make sure libvpic_hip.so is built
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "plumbing16")])
    run_deck([str(tmp_path / "plumbing16.hip.exe"), "-tpp=1"], cwd=tmp_path,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    en = np.loadtxt(tmp_path / "energies16.txt")
    ref = gold["energies_1rank"]
    assert en.shape[0] == ref.shape[0] == 51 and np.array_equal(en[:, 0], np.arange(51))
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=2e-7)           # kinetic energy
    np.testing.assert_allclose(en[1:, 1:7], ref[1:, :6], rtol=5e-4)      # field energies
    sys.path.insert(0, ROOT)
    from oracle import deck16
    _, f0, p0 = deck16.read_state(tmp_path / "state16_step0_rank0.bin")
    mine = deck16.load_particles()
    order = np.argsort(p0["tag"])
    for n in ("dx", "dy", "dz", "i", "ux", "uy", "uz", "q"):              # the deck's loader ran unchanged
        assert np.array_equal(p0[n][order], mine[n]), n
    _, f50, p50 = deck16.read_state(tmp_path / "state16_step50_rank0.bin")
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
        scale = max(np.abs(gold["f50_" + k]).max() for k in (("ex", "ey", "ez") if c[0] == "e" else ("cbx", "cby", "cbz")))
        assert np.abs(f50[c] - gold["f50_" + c]).max() <= 2e-4 * scale, c
    assert np.abs(np.bincount(p50["i"], minlength=len(f50)) - gold["p50_cell_count"]).sum() <= 4


def test_reference_deck_with_divergence_cleaning(tmp_path):
    """The same deck with -DCLEAN_INTERVAL=10: initialize()'s derived fields (rhob at step 0) and
    advance()'s cleaning / synchronisation sections (advance.cxx:151-208) run on the HIP path."""
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "DECK_DEFS=-DCLEAN_INTERVAL=10",
                           "OUT=" + str(tmp_path / "plumbing16c")])
    # the FLOAT mode, asked for: decks that clean div E run with deterministic sums by default since round 4 (next test)
    run_deck([str(tmp_path / "plumbing16c.hip.exe"), "-tpp=1"], cwd=tmp_path, env=dict(os.environ, VPIC_HIP_DETERMINISTIC="0"),
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    en = np.loadtxt(tmp_path / "energies16.txt")
    ref = gold["clean_energies_1rank"]
    # rhof is summed by float atomics (order varies from run to run), and the Marder pass feeds it back
    # into E every 10 steps: the kinetic energy follows to ~3e-7 instead of the 2e-7 of the plain deck
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=1e-6)
    np.testing.assert_allclose(en[1:, 1:7], ref[1:, :6], rtol=5e-4)
    sys.path.insert(0, ROOT)
    from oracle import deck16
    _, f0, _ = deck16.read_state(tmp_path / "state16_step0_rank0.bin")
    r0 = gold["clean_f0_rhob"]
    assert np.abs(f0["rhob"] - r0).max() <= 2e-6 * np.abs(r0).max()      # accumulate_rho_p sums by float atomics
    _, f50, _ = deck16.read_state(tmp_path / "state16_step50_rank0.bin")
    # Two outcomes occur, about 2:1 (tools/deck_flaky.py, tools/dbg_clean_flaky.py): in one of them a
    # particle that ends step 9 within round-off of a cell face lands on the other side of it than
    # in the reference run (rhof's float-atomic summation order perturbs E by ~1e-7 through the
    # Marder pass), is interpolated from the neighbouring cell from then on, and the runs drift
    # apart to ~7e-4 of the field scale by step 50.  In both, every advance_p launch agrees with the
    # oracle run on that launch's own inputs to 3e-9 and bit for bit in the particles.
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
        scale = max(np.abs(gold["clean_f50_" + k]).max() for k in (("ex", "ey", "ez") if c[0] == "e" else ("cbx", "cby", "cbz")))
        assert np.abs(f50[c] - gold["clean_f50_" + c]).max() <= 2e-3 * scale, c
    assert np.abs(f50["rhob"] - gold["clean_f50_rhob"]).max() <= 2e-6 * np.abs(r0).max()
    assert np.abs(f50["rhof"] - gold["clean_f50_rhof"]).max() <= 4e-3 * np.abs(gold["clean_f50_rhof"]).max()
    assert np.abs(f50["div_e_err"]).max() <= 1e-5 and np.abs(f50["div_b_err"]).max() <= 1e-5


def test_cleaning_deck_is_reproducible_in_deterministic_mode(tmp_path):
    """VPIC_HIP_DETERMINISTIC=1 (vpic_hip_set_accumulation: 64-bit fixed-point sums for the accumulators and for rhof): two
    runs of the cleaning deck -- the one whose float-atomic runs fall into two groups, see above -- write the SAME bytes,
    as two runs of the reference do (reduce_accumulators.cxx:37-55 sums in a fixed order).  Against the reference's run the
    one outcome there is now is held to the plain deck's field tolerance."""
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "DECK_DEFS=-DCLEAN_INTERVAL=10",
                           "OUT=" + str(tmp_path / "plumbing16c")])
    env = dict(os.environ, VPIC_HIP_DETERMINISTIC="1")
    default = {k: v for k, v in os.environ.items() if k != "VPIC_HIP_DETERMINISTIC"}     # unset: a deck that cleans div E gets the mode by itself
    out = []
    for run in ("a", "b", "c"):
        d = tmp_path / run
        d.mkdir()
        run_deck([str(tmp_path / "plumbing16c.hip.exe"), "-tpp=1"], cwd=d, env=default if run == "c" else env,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    sys.path.insert(0, ROOT)
    from oracle import deck16
    for run in ("a", "b", "c"):
        _, f, p = deck16.read_state(tmp_path / run / "state16_step50_rank0.bin")
        out.append((f, p[np.argsort(p["tag"], kind="stable")], np.loadtxt(tmp_path / run / "energies16.txt")))
    for f, p, en in out[1:]:
        # the fields to the last bit, the particles to the last bit (their ORDER in the array is the sort's atomics' and
        # differs; so do the energy sums, in the sixteenth digit: they are added in array order)
        assert f.tobytes() == out[0][0].tobytes(), "the fields of two deterministic runs differ"
        assert p.tobytes() == out[0][1].tobytes(), "the particles of two deterministic runs differ"
        np.testing.assert_allclose(en, out[0][2], rtol=1e-12, atol=0)
    f50 = out[0][0]
    en = np.loadtxt(tmp_path / "a" / "energies16.txt")
    np.testing.assert_allclose(en[:, 7], gold["clean_energies_1rank"][:, 6], rtol=1e-6)
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
        scale = max(np.abs(gold["clean_f50_" + k]).max() for k in (("ex", "ey", "ez") if c[0] == "e" else ("cbx", "cby", "cbz")))
        assert np.abs(f50[c] - gold["clean_f50_" + c]).max() <= 2e-4 * scale, c


def test_reference_deck_binary_dumps(tmp_path):
    """-DWRITE_DUMPS: dump_fields / dump_hydro / dump_particles at step 10 (dump.cxx:190-329).  Headers
    byte for byte; payloads within the tolerances of a state that went through 10 steps."""
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "DECK_DEFS=-DWRITE_DUMPS", "OUT=" + str(tmp_path / "plumbing16d")])
    run_deck([str(tmp_path / "plumbing16d.hip.exe"), "-tpp=1"], cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    L = importlib.import_module("old-vpic_amd.layout")
    for name in ("fields16", "hydro16", "particles16"):
        head = gold["dump_" + name + "_head"]
        raw = np.fromfile(tmp_path / (name + ".10.0"), np.uint8)
        assert np.array_equal(raw[:len(head)], head), name            # V0 header + array header, exact
    nh = len(gold["dump_fields16_head"])
    f = np.fromfile(tmp_path / "fields16.10.0", L.field_t, offset=nh)
    ref = gold["dump_fields16"]
    assert len(f) == len(ref)
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz", "jfx", "jfy", "jfz", "rhob"):
        scale = max(np.abs(ref[c]).max(), 1e-12)
        assert np.abs(f[c] - ref[c]).max() <= 2e-5 * scale, c
    h = np.fromfile(tmp_path / "hydro16.10.0", L.hydro_t, offset=nh)
    rh = gold["dump_hydro16"]
    for c in h.dtype.names[:-1]:
        assert np.abs(h[c] - rh[c]).max() <= 2e-5 * np.abs(rh[c]).max(), c
    p = np.fromfile(tmp_path / "particles16.10.0", L.particle_t, offset=len(gold["dump_particles16_head"]))
    assert len(p) == int(gold["dump_particles16_n"])
    sub, rs = p[np.argsort(p["tag"])][::16], gold["dump_particles16_sub"]
    assert np.array_equal(sub["tag"], rs["tag"]) and (sub["i"] != rs["i"]).mean() < 1e-3
    same = sub["i"] == rs["i"]
    for c in ("dx", "dy", "dz", "ux", "uy", "uz"):
        assert np.abs(sub[c][same] - rs[c][same]).max() <= 2e-5, c
    # text and grid dumps (dump.cxx:82-187): the reference's bytes
    for name in ("species16.txt", "materials16.txt", "global16.vpc", "grid16.0"):
        assert np.array_equal(np.fromfile(tmp_path / name, np.uint8), gold["dump_" + name]), name
    # field_dump / hydro_dump (dump.cxx:1116-1552): headers are the reference's bytes; the payload, gathered
    # on the device, is exactly the banded / strided rearrangement of the state that dump_fields wrote at
    # the same step (byte work: bit-exact), and for hydro of a moment array accumulated afresh by float
    # atomics (summation order differs between two accumulations: 2e-6 of the largest entry)
    sys.path.insert(0, ROOT)
    from oracle import deck16, dumpfmt as D
    H = D.HEADER_V0 + 8 + 12
    for name, kind, layout, words, strides in deck16.DUMP_CASES:
        raw = np.fromfile(tmp_path / "T.10" / (name + ".10.0"), np.uint8)
        assert np.array_equal(raw[:H], gold["dump_" + name + "_head"]), name
        got = raw[H:].view(np.uint32)
        want = D.gather(f if kind == "f" else h, 16, 16, 16, layout, words, strides).ravel()
        assert got.shape == want.shape, name
        if kind == "f":
            assert np.array_equal(got, want), name
        else:
            a, b = got.view(np.float32).astype(np.float64), want.view(np.float32).astype(np.float64)
            assert np.abs(a - b).max() <= 2e-6 * np.abs(b).max(), name


def test_reference_deck_on_two_mpi_ranks(tmp_path):
    """The same deck file on TWO ranks of the HIP host (make MPI=1; both ranks share the one GPU of the
    box): x-slabs, ghost / current / particle exchanges over MPI, against the reference's own 2-rank run."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "MPI=1", "DECK=" + deck, "OUT=" + str(tmp_path / "plumbing16m")])
    run_deck([mpiexec, "-n", "2", str(tmp_path / "plumbing16m.hip.exe"), "-tpp=1"], cwd=tmp_path,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    en = np.loadtxt(tmp_path / "energies16.txt")
    ref = gold["energies_2rank"]
    assert en.shape[0] == 51
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=2e-7)           # kinetic energy (global sum)
    np.testing.assert_allclose(en[1:, 1:7], ref[1:, :6], rtol=5e-4)      # field energies
    sys.path.insert(0, ROOT)
    from oracle import deck16
    # the two slabs together hold every particle, each in its own half of the box
    n = 0
    for r in range(2):
        dims, f50, p50 = deck16.read_state(tmp_path / ("state16_step50_rank%d.bin" % r))
        assert dims == (8, 16, 16)
        n += len(p50)
        x = f50.reshape(18, 18, 10)
        ref_c = gold["f50_ex"].reshape(18, 18, 18)[:, :, 1 + 8 * r:9 + 8 * r]
        scale = np.abs(gold["f50_ex"]).max()
        assert np.abs(x["ex"][:, :, 1:9] - ref_c).max() <= 2e-3 * scale     # the 1-rank reference fields, slab by slab
    assert n == 16 * 16 * 16 * 8


def test_reference_deck_with_cleaning_on_two_mpi_ranks(tmp_path):
    """Two ranks with -DCLEAN_INTERVAL=10: rho / normal-E / div-B / tang-E-norm-B planes cross the slab
    boundary over MPI.  Against the reference's 1-rank run of the same deck (its own 1- vs 2-rank runs
    differ by 1e-9 in energy on the plain deck)."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "MPI=1", "DECK_DEFS=-DCLEAN_INTERVAL=10", "DECK=" + deck, "OUT=" + str(tmp_path / "plumbing16mc")])
    run_deck([mpiexec, "-n", "2", str(tmp_path / "plumbing16mc.hip.exe"), "-tpp=1"], cwd=tmp_path,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    en = np.loadtxt(tmp_path / "energies16.txt")
    ref = gold["clean_energies_1rank"]
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=1e-6)
    np.testing.assert_allclose(en[1:, 1:7], ref[1:, :6], rtol=5e-4)
    sys.path.insert(0, ROOT)
    from oracle import deck16
    r0 = gold["clean_f0_rhob"].reshape(18, 18, 18)
    for r in range(2):
        _, f0, _ = deck16.read_state(tmp_path / ("state16_step0_rank%d.bin" % r))
        got = f0["rhob"].reshape(18, 18, 10)[1:17, 1:17, 1:9]
        assert np.abs(got - r0[1:17, 1:17, 1 + 8 * r:9 + 8 * r]).max() <= 2e-6 * np.abs(r0).max()


def test_reference_deck_dumps_on_two_mpi_ranks(tmp_path):
    """-DWRITE_DUMPS on two ranks: dump_grid in the reference's global cell numbering (ops.c:52-97,135-182)
    byte for byte, and a banded hydro_dump whose moments were summed across the slab boundary over MPI
    (hydro.c:28-163), against the files of the reference's own 2-rank run."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "MPI=1", "DECK_DEFS=-DWRITE_DUMPS", "DECK=" + deck, "OUT=" + str(tmp_path / "plumbing16md")])
    run_deck([mpiexec, "-n", "2", str(tmp_path / "plumbing16md.hip.exe"), "-tpp=1"], cwd=tmp_path,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    sys.path.insert(0, ROOT)
    from oracle import dumpfmt as D
    H = D.HEADER_V0 + 8 + 12
    for r in range(2):
        assert np.array_equal(np.fromfile(tmp_path / ("grid16.%d" % r), np.uint8), gold["dump2_grid16.%d" % r]), r
        raw, ref = np.fromfile(tmp_path / "T.10" / ("hband.10.%d" % r), np.uint8), gold["dump2_hband_%d" % r]
        assert np.array_equal(raw[:H], ref[:H]), r
        a = raw[H:].view(np.float32).reshape(-1, 18, 6, 6).astype(np.float64)       # [word][z][y/4+2][x/2+2] of an 8x16x16 slab
        b = ref[H:].view(np.float32).reshape(a.shape).astype(np.float64)
        for w in range(a.shape[0]):
            assert np.abs(a[w] - b[w]).max() <= 2e-5 * np.abs(b[w]).max(), (r, w)


def _sheet4_check(tmp_path, gold, key, nranks, migrating=False):
    # migrating: one rank that sends to itself across its periodic axes -- particles that wrap travel as injector records, like the
    # migrants of a several-rank run (tags: see below)
    """Outputs of oracle/decks/sheet4.cxx on the HIP host against the reference executable's (tests/golden/
    sheet4.npz).  Both load bit-identical particles (normals are drawn inside the deck), so differences
    are fp32 summation order amplified by 40 steps of a hot (vth 0.25 c), wall-bounded plasma."""
    sys.path.insert(0, ROOT)
    from oracle import dumpfmt as D, sheet4 as S
    L = importlib.import_module("old-vpic_amd.layout")
    dev = {}
    for name in ("global.vpc", "rundata/species", "rundata/materials"):
        assert np.array_equal(np.fromfile(tmp_path / name, np.uint8), gold[key + name]), name
    en, ref = np.loadtxt(tmp_path / "energies4.txt"), gold[key + "energies"]
    assert en.shape == ref.shape == (S.STEPS + 1, 11)
    np.testing.assert_allclose(en[0, 4:], ref[0, 4:], rtol=2e-7)                 # the load and the initial field: identical states
    np.testing.assert_allclose(en[:, 7:], ref[:, 7:], rtol=2e-5)                 # kinetic energy of each species, every step
    np.testing.assert_allclose(en[:, 4:6], ref[:, 4:6], rtol=2e-5)               # the sheet's magnetic energy (x, y)
    scale = ref[:, 1:7].max()
    assert np.abs(en[:, 1:7] - ref[:, 1:7]).max() <= 2e-5 * scale                # the small components, against the largest
    dev["ke"] = np.abs(en[:, 7:] / ref[:, 7:] - 1).max(); dev["fe"] = np.abs(en[:, 1:7] - ref[:, 1:7]).max() / scale
    txt = np.loadtxt(tmp_path / "rundata" / "energies", comments="%")             # dump_energies (dump.cxx:37-77), %e precision
    rtxt = np.loadtxt(__import__("io").BytesIO(gold[key + "rundata/energies"].tobytes()), comments="%")
    assert txt.shape == rtxt.shape and np.array_equal(txt[:, 0], rtxt[:, 0])
    np.testing.assert_allclose(txt[:, 4:], rtxt[:, 4:], rtol=3e-5)
    H = D.HEADER_V0 + 8 + 12
    nxl = S.NX // nranks
    for r in range(nranks):
        k = key + "r%d_" % r
        assert np.array_equal(np.fromfile(tmp_path / "rundata" / ("grid.%d" % r), np.uint8), gold[k + "grid"]), r
        for what, path, nw, dims in (("field_dump", "fields/T.%d/fields.%d.%d", 9, (S.NZ // 2 + 2, S.NY + 2, nxl // 2 + 2)),
                                     ("hydro_dump", "hydro/T.%d/eThydro.%d.%d", 4, (S.NZ + 2, S.NY + 2, nxl + 2))):
            raw, rr = np.fromfile(tmp_path / (path % (S.DUMP_STEP, S.DUMP_STEP, r)), np.uint8), gold[k + what]
            assert np.array_equal(raw[:H], rr[:H]), (what, r)                     # V0 header + array header: the reference's bytes
            a = raw[H:].view(np.float32).reshape((nw,) + dims).astype(np.float64)
            b = rr[H:].view(np.float32).reshape(a.shape).astype(np.float64)
            group = 3 if what == "field_dump" else 4                               # E, B, J share a scale; so do the moments
            for g0 in range(0, nw, group):
                s = np.abs(b[g0:g0 + group]).max()
                d = np.abs(a[g0:g0 + group] - b[g0:g0 + group]).max() / s
                dev["%s_%d_r%d" % (what, g0, r)] = d
                assert d <= (5e-3 if what == "field_dump" else 2e-2), (what, g0, r, d)
        f = np.fromfile(tmp_path / ("fields4_rank%d.bin" % r), L.field_t, (nxl + 2) * (S.NY + 2) * (S.NZ + 2))
        counts = np.fromfile(tmp_path / ("fields4_rank%d.bin" % r), np.int32, 4, offset=f.nbytes)
        bscale = max(np.abs(gold[k + "f_" + c]).max() for c in ("cbx", "cby", "cbz"))
        for c in ("cbx", "cby", "cbz", "ex", "ey", "ez"):
            d = np.abs(f[c] - gold[k + "f_" + c]).max() / bscale
            dev["f_%s_r%d" % (c, r)] = d
            # run-to-run the deviations fall into two groups, 1e-5..1e-4 and 1e-3..2.4e-3, each reproduced digit for
            # digit (tools/sheet4_spread.sh): a particle that ends a step within round-off of a cell face goes one
            # way or the other depending on the summation order of the float atomics, and its deposit differs by a
            # whole cell from then on -- the per-cell interpolator makes that a finite jump.  Both are runs the
            # reference's arithmetic allows; the bound covers the second group.
            assert d <= 5e-3, (c, r, d)
        if nranks == 1:
            assert np.array_equal(counts, gold[k + "np"])                        # nothing leaves a one-rank box
        else:
            assert np.abs(counts - gold[k + "np"]).max() <= 8, (counts, gold[k + "np"])   # a handful of face-grazing crossings may differ
        tr = S.read_tracers(tmp_path / ("tracers4_rank%d.bin" % r))
        for name, t in zip(("iR", "eR"), tr):
            want = gold[k + "tracers_" + name]
            t = t[np.argsort(t["tag"])]
            if nranks == 1 and not migrating:
                assert np.array_equal(t["tag"], want["tag"]), name
            else:
                # A particle that migrates travels as an injector record, which has no tag fields: on arrival it
                # takes whatever tag the array slot held (boundary_p.c:477-496), here as in the reference.  Compare
                # the tracers whose tag is unique on this rank in both runs (those that stayed), and the head count.
                assert abs(len(t) - len(want)) <= 0.02 * len(want), (name, len(t), len(want))
                ut, ct = np.unique(t["tag"], return_counts=True)
                uw, cw = np.unique(want["tag"], return_counts=True)
                both = np.intersect1d(ut[ct == 1], uw[cw == 1])
                # (one rank sending to itself: every wrap around the small periodic box is a migration, most tracers make one in 40 steps)
                assert len(both) >= (0.25 if migrating else 0.5) * len(want), (name, len(both), len(want))
                t, want = t[np.isin(t["tag"], both)], want[np.isin(want["tag"], both)]
                dev["tracer_matched_%s_r%d" % (name, r)] = len(both) / len(gold[k + "tracers_" + name])
            assert np.all(t["q"] == 0)
            same = t["i"] == want["i"]
            dev["tracer_cell_%s_r%d" % (name, r)] = 1 - same.mean()
            assert same.mean() >= 0.98, (name, r, same.mean())
            for c in ("ux", "uy", "uz"):
                d = np.abs(t[c] - want[c])
                dev["tracer_%s_%s_r%d" % (c, name, r)] = np.median(d)
                assert np.median(d) <= 1e-4 and np.quantile(d, 0.99) <= 2e-2, (name, c, np.median(d), np.quantile(d, 0.99))
    out = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, "sheet4_dev_%s.txt" % key), "w") as fh:
            for k2 in sorted(dev):
                fh.write("%s %.3e\n" % (k2, dev[k2]))


def test_sheet_deck_with_tracers(tmp_path):
    """A reconnection-style deck (oracle/decks/sheet4.cxx): 4 species + 2 tracer species that the DECK
    advances through advance_p / boundary_p / sort_p (served by the resident engine), PEC z walls with
    reflecting particles, set_region_field, cleaning every 10 steps, DumpParameters / FileIO / turnstile."""
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "sheet4.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "sheet4")])
    run_deck([str(tmp_path / "sheet4.hip.exe"), "-tpp=1"], cwd=tmp_path, stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL, timeout=300)
    _sheet4_check(tmp_path, np.load(os.path.join(ROOT, "tests", "golden", "sheet4.npz")), "n1_", 1)


def test_sheet_deck_with_tracers_on_two_mpi_ranks(tmp_path):
    """The same deck on two x-slabs: tracers and plasma cross the slab boundary through the one exchange
    of the main loop; against the reference's own 2-rank run (per-rank seeds: its own particle load)."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "sheet4.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "MPI=1", "DECK=" + deck, "OUT=" + str(tmp_path / "sheet4m")])
    run_deck([mpiexec, "-n", "2", str(tmp_path / "sheet4m.hip.exe"), "-tpp=1"], cwd=tmp_path,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    _sheet4_check(tmp_path, np.load(os.path.join(ROOT, "tests", "golden", "sheet4.npz")), "n2_", 2)


@pytest.mark.parametrize("nranks", [1, 2])
def test_restart_continues_the_run(tmp_path, nranks):
    """dump_restart at step 20 of the plumbing deck, then `deck.exe restart restart16` (dump.cxx:332-851,
    main.cxx:83-86): the restarted run writes steps 21..50 again; they must repeat the uninterrupted run's
    (same particle order, same fields; float-atomic summation order is all that differs)."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if nranks > 1 and not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    exe = str(tmp_path / "plumbing16r")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK_DEFS=-DRESTART_AT=20", "DECK=" + deck, "OUT=" + exe]
                          + (["MPI=1"] if nranks > 1 else []))
    launch = [mpiexec, "-n", str(nranks)] if nranks > 1 else []
    quiet = dict(cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    run_deck(launch + [exe + ".hip.exe", "-tpp=1"], **quiet)
    first = np.loadtxt(tmp_path / "energies16.txt")
    assert first.shape[0] == 51 and all((tmp_path / ("restart16.%d" % r)).exists() for r in range(nranks))
    run_deck(launch + [exe + ".hip.exe", "restart", "restart16"], **quiet)
    both = np.loadtxt(tmp_path / "energies16.txt")
    again = both[51:]
    assert again.shape[0] == 30 and np.array_equal(again[:, 0], np.arange(21, 51))
    np.testing.assert_allclose(again[:, 7], first[21:, 7], rtol=1e-6)            # kinetic energy
    np.testing.assert_allclose(again[:, 1:7], first[21:, 1:7], rtol=2e-3)        # field energies (small, chaotic)
    # ... and the REFERENCE's uninterrupted run of the same deck (tests/golden/deck16.npz, its own executable on the same
    # number of ranks): the steps after the restart are held to the plain deck's tolerances against it, so a restart
    # that dropped or altered state cannot hide behind a comparison of the host with itself
    ref = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))["energies_%drank" % nranks]
    np.testing.assert_allclose(again[:, 7], ref[21:, 6], rtol=2e-7 if nranks == 1 else 1e-6)
    np.testing.assert_allclose(again[:, 1:7], ref[21:, :6], rtol=1e-3)


def test_reference_deck_with_materials(tmp_path):
    """-DMATERIALS: a dielectric / magnetic slab and a block of anisotropic conductor, set with the deck's
    define_material (both overloads) and set_region_material (deck_wrapper.cxx:228-278, sfa.c:145-177).
    The material ids every voxel ends up with are the reference's exactly; energies and fields after 50
    steps within the plain deck's tolerances."""
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "DECK_DEFS=-DMATERIALS", "OUT=" + str(tmp_path / "plumbing16x")])
    run_deck([str(tmp_path / "plumbing16x.hip.exe"), "-tpp=1"], cwd=tmp_path, stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL, timeout=300)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    sys.path.insert(0, ROOT)
    from oracle import deck16
    _, f0, _ = deck16.read_state(tmp_path / "state16_step0_rank0.bin")
    for c in ("ematx", "ematy", "ematz", "nmat", "fmatx", "fmaty", "fmatz", "cmat"):
        assert np.array_equal(f0[c], gold["mat_f0_" + c]), c
    en, ref = np.loadtxt(tmp_path / "energies16.txt"), gold["mat_energies_1rank"]
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=2e-7)
    np.testing.assert_allclose(en[1:, 1:7], ref[1:, :6], rtol=5e-4)
    _, f50, _ = deck16.read_state(tmp_path / "state16_step50_rank0.bin")
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
        scale = np.abs(gold["mat_f50_" + c]).max()
        assert np.abs(f50[c] - gold["mat_f50_" + c]).max() <= 2e-3 * scale, c


@pytest.mark.parametrize("nranks", [1, 2])
def test_reference_deck_open_box(tmp_path, nranks):
    """-DABSORBING: define_absorbing_grid with absorb_particles (partition.c:86-137): Higdon field absorption on
    every outer face, particles leaving through them are removed and their charge left in rhob
    (boundary_p.c:9-71).  Particle head counts must be the reference's exactly; energies and fields close."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if nranks > 1 and not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    exe = str(tmp_path / "plumbing16o")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK_DEFS=-DABSORBING", "DECK=" + deck, "OUT=" + exe]
                          + (["MPI=1"] if nranks > 1 else []))
    launch = [mpiexec, "-n", str(nranks)] if nranks > 1 else []
    run_deck(launch + [exe + ".hip.exe", "-tpp=1"], cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    sys.path.insert(0, ROOT)
    from oracle import deck16
    en, ref = np.loadtxt(tmp_path / "energies16.txt"), gold["abs%d_energies" % nranks]
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=1e-5)           # one particle leaving a step earlier or later is 4e-5 of the total
    np.testing.assert_allclose(en[1:, 1:7], ref[1:, :6], rtol=2e-3)
    for r in range(nranks):
        _, f50, p50 = deck16.read_state(tmp_path / ("state16_step50_rank%d.bin" % r))
        assert abs(len(p50) - int(gold["abs%d_np_r%d" % (nranks, r)])) <= 2, r   # exact in every run so far; a face-grazing particle may differ
        for c in ("ex", "cby", "rhob"):
            want = gold["abs%d_f50_%s_r%d" % (nranks, c, r)]
            assert np.abs(f50[c] - want).max() <= 2e-3 * np.abs(want).max(), (c, r)


@pytest.mark.parametrize("nranks", [1, 2])
def test_reference_deck_with_runtime_injection(tmp_path, nranks):
    """-DINJECT: 24 particles per step come in through inject_particle from begin_particle_injection
    (misc.cxx:16-105 with age 0): they join the device species when the deck's call returns, are pushed from the
    next step on, and a rank keeps exactly the ones inside its domain."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if nranks > 1 and not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    exe = str(tmp_path / "plumbing16i")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK_DEFS=-DINJECT", "DECK=" + deck, "OUT=" + exe]
                          + (["MPI=1"] if nranks > 1 else []))
    launch = [mpiexec, "-n", str(nranks)] if nranks > 1 else []
    run_deck(launch + [exe + ".hip.exe", "-tpp=1"], cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    sys.path.insert(0, ROOT)
    from oracle import deck16
    en, ref = np.loadtxt(tmp_path / "energies16.txt"), gold["inj%d_energies" % nranks]
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=5e-7)
    np.testing.assert_allclose(en[1:, 1:7], ref[1:, :6], rtol=1e-3)
    states = [deck16.read_state(tmp_path / ("state16_step50_rank%d.bin" % r)) for r in range(nranks)]
    parts = [st[2] for st in states]
    assert sum(len(p) for p in parts) == int(gold["inj%d_np" % nranks])
    # every other injected particle was injected with update_rhob: its charge, negated, sits in rhob (misc.cxx:87-91)
    rhob, want = np.concatenate([st[1]["rhob"] for st in states]), gold["inj%d_rhob" % nranks]
    assert np.abs(rhob - want).max() <= 1e-5 * np.abs(want).max()
    if nranks == 1:                                          # tags survive on one rank: the fed-in particles one by one
        fed, want = parts[0][parts[0]["tag"] >= 1000000], gold["inj1_fed"]
        fed = fed[np.argsort(fed["tag"])]
        assert np.array_equal(fed["tag"], want["tag"])
        assert (fed["i"] == want["i"]).mean() >= 0.995
        for c in ("ux", "uy", "uz"):
            assert np.median(np.abs(fed[c] - want[c])) <= 1e-5, c


@pytest.mark.parametrize("nranks", [1, 2])
def test_reference_deck_with_field_injection_hook(tmp_path, nranks):
    """-DANTENNA: begin_field_injection edits E in place every step (advance.cxx:141).  The host arrays a deck
    sees are mirrors of device state kept coherent on demand (page protection: the first touch of an array in
    a hook brings it over, what the hook wrote goes back when it returns), so the unchanged deck drives the
    plasma exactly as it drives the reference's: the energy it pumps in (16 -> 66 in 50 steps) must match."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if nranks > 1 and not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    exe = str(tmp_path / "plumbing16a")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK_DEFS=-DANTENNA", "DECK=" + deck, "OUT=" + exe]
                          + (["MPI=1"] if nranks > 1 else []))
    launch = [mpiexec, "-n", str(nranks)] if nranks > 1 else []
    run_deck(launch + [exe + ".hip.exe", "-tpp=1"], cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    en, ref = np.loadtxt(tmp_path / "energies16.txt"), gold["ant%d_energies" % nranks]
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=2e-6)
    np.testing.assert_allclose(en[1:, 1:7], ref[1:, :6], rtol=2e-4)


@pytest.mark.parametrize("tag,defs", [("t221", "-DTOPO_Y=2 -DCLEAN_INTERVAL=10 -DWRITE_DUMPS"), ("t122", "-DTOPO_Y=2 -DTOPO_Z=2"),
                                      ("t221abs", "-DTOPO_Y=2 -DABSORBING")])
def test_reference_deck_on_bricks(tmp_path, tag, defs):
    """Four ranks as 2x2x1 and 1x2x2 bricks (partition.c:35-131, RANK_TO_INDEX): every exchange runs axis by axis
    -- x, then y, then z, so that edges and corners propagate (remote.c:284-289) -- over whichever faces are
    shared; with cleaning and the dumps (global cell numbering of dump_grid across y faces, hydro summed across
    them), and as an open box.  Against the reference's own 4-rank runs of the same topologies."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    exe = str(tmp_path / ("plumbing16" + tag))
    subprocess.check_call(["make", "-s", "-C", host, "deck", "MPI=1", "DECK_DEFS=" + defs, "DECK=" + deck, "OUT=" + exe])
    run_deck([mpiexec, "-n", "4", exe + ".hip.exe", "-tpp=1"], cwd=tmp_path, stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL, timeout=600)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    sys.path.insert(0, ROOT)
    from oracle import deck16, dumpfmt as D
    en, ref = np.loadtxt(tmp_path / "energies16.txt"), gold[tag + "_energies"]
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=1e-6)
    np.testing.assert_allclose(en[1:, 1:7], ref[1:, :6], rtol=2e-3)
    counts = np.array([len(deck16.read_state(tmp_path / ("state16_step50_rank%d.bin" % r))[2]) for r in range(4)])
    if tag == "t221abs":
        assert np.abs(counts - gold[tag + "_np"]).max() <= 4 and abs(int(counts.sum()) - int(gold[tag + "_np"].sum())) <= 4
    else:
        assert counts.sum() == gold[tag + "_np"].sum() and np.abs(counts - gold[tag + "_np"]).max() <= 4
    if tag == "t221":
        H = D.HEADER_V0 + 8 + 12
        for r in range(4):
            assert np.array_equal(np.fromfile(tmp_path / ("grid16.%d" % r), np.uint8), gold["t221_grid16.%d" % r]), r
            raw, want = np.fromfile(tmp_path / "T.10" / ("hband.10.%d" % r), np.uint8), gold["t221_hband_%d" % r]
            assert np.array_equal(raw[:H], want[:H]), r
            a, b = raw[H:].view(np.float32).astype(np.float64), want[H:].view(np.float32).astype(np.float64)
            assert np.abs(a - b).max() <= 2e-4 * np.abs(b).max(), r


@pytest.mark.parametrize("nranks", [1, 2])
def test_reference_deck_with_reflux_walls(tmp_path, nranks):
    """-DREFLUX: add_boundary( grid, maxwellian_reflux, &params ) on the z walls (boundary/maxwellian_reflux.c,
    grid/add_boundary.c).  The handler draws random numbers, the device from its own counter-based stream: the
    comparison is statistical.  The reference's 1- and 2-rank runs differ by 6e-4 in kinetic energy and up to
    6e-3 in the momentum moments for the same reason; the bounds are five times that.  No particle may be lost."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if nranks > 1 and not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    exe = str(tmp_path / "plumbing16f")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK_DEFS=-DREFLUX", "DECK=" + deck, "OUT=" + exe]
                          + (["MPI=1"] if nranks > 1 else []))
    launch = [mpiexec, "-n", str(nranks)] if nranks > 1 else []
    run_deck(launch + [exe + ".hip.exe", "-tpp=1"], cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    sys.path.insert(0, ROOT)
    from oracle import deck16
    en, ref = np.loadtxt(tmp_path / "energies16.txt"), gold["rfx%d_energies" % nranks]
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=3e-3)
    assert ref[-1, 6] < 0.93 * ref[0, 6]                           # the walls do cool the beams: the handler matters
    parts = np.concatenate([deck16.read_state(tmp_path / ("state16_step50_rank%d.bin" % r))[2] for r in range(nranks)])
    assert len(parts) == int(gold["rfx%d_np" % nranks]) == 16 ** 3 * 8
    u2 = np.array([np.mean(parts[c].astype(np.float64) ** 2) for c in ("ux", "uy", "uz")])
    np.testing.assert_allclose(u2, gold["rfx%d_u2" % nranks], rtol=5e-2)       # (per particle: tests/test_gpu_kernels.py::test_maxwellian_reflux_particle_by_particle)


@pytest.mark.parametrize("nranks", [1, 2])
def test_reference_deck_with_emitter(tmp_path, nranks):
    """-DEMITTER: define_surface_emitter( "cathode", electron, child_langmuir, z<2 ) in a uniform E_z
    (src/emitter/child-langmuir.c, deck_wrapper.cxx:389-463, advance.cxx:83-84): the emitting faces, the charge
    law, the half-Maxwellian momenta, the random ages, the bound charge left behind.  The model draws random
    numbers (the device its own): statistical comparison; the reference's 1- and 2-rank runs differ by 2e-4 in
    the particle count and 6e-4 in energies and bound charge; bounds are five times that."""
    mpiexec = "/opt/conda/bin/mpiexec"
    if nranks > 1 and not os.path.exists(mpiexec):
        pytest.skip("no MPI launcher on this box")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "oracle", "decks", "plumbing16.cxx")
    exe = str(tmp_path / "plumbing16e")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK_DEFS=-DEMITTER", "DECK=" + deck, "OUT=" + exe]
                          + (["MPI=1"] if nranks > 1 else []))
    launch = [mpiexec, "-n", str(nranks)] if nranks > 1 else []
    run_deck(launch + [exe + ".hip.exe", "-tpp=1"], cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "deck16.npz"))
    sys.path.insert(0, ROOT)
    from oracle import deck16
    en, ref = np.loadtxt(tmp_path / "energies16.txt"), gold["emit%d_energies" % nranks]
    np.testing.assert_allclose(en[:, 7], ref[:, 6], rtol=5e-3)           # kinetic energy: 16 -> 127, the emitted charge falling through E_z (the emitted particles are drawn from the device's own stream: a statistical comparison)
    assert np.abs(en[:, 3] - ref[:, 2]).max() <= 3e-3 * ref[:, 2].max()   # E_z energy: 184 -> 7 -> 73, a plasma oscillation
    st = [deck16.read_state(tmp_path / ("state16_step50_rank%d.bin" % r)) for r in range(nranks)]
    parts = np.concatenate([x[2] for x in st])
    assert abs(len(parts) - int(gold["emit%d_np" % nranks])) <= 1e-3 * int(gold["emit%d_np" % nranks])
    rhob = sum(x[1]["rhob"].astype(np.float64).reshape(18, 18, -1)[1:17, 1:17, 1:-1].sum() for x in st)
    assert abs(rhob - float(gold["emit%d_rhob_sum" % nranks])) <= 3e-3 * abs(float(gold["emit%d_rhob_sum" % nranks]))
    if nranks == 1:
        new = parts[parts["tag"] == 0]
        assert abs(new["q"].astype(np.float64).sum() - float(gold["emit1_q_sum"])) <= 3e-3 * abs(float(gold["emit1_q_sum"]))
        u2 = np.array([np.mean(new[c].astype(np.float64) ** 2) for c in ("ux", "uy", "uz")])
        # along the field 1 %; across it the momenta are 4e-4 from the emission law plus 6e-4 of heating by the
        # noise fields E_x, E_y, whose energies themselves differ by 10 % between two runs with different random numbers
        np.testing.assert_allclose(u2[2], gold["emit1_u2"][2], rtol=2e-2)
        np.testing.assert_allclose(u2[:2], gold["emit1_u2"][:2], rtol=0.2)


@pytest.mark.parametrize("nranks", [1, 2])
def test_production_reconnection_deck(tmp_path, nranks):
    """oracle/_ref/trecon{1,2}.hip.exe: the reference's production deck decks/trecon-part/turbulence.cxx (+ tracer.cxx,
    energy.cxx: 1.8 k lines, UNCHANGED; BASELINE configs[3] in small: oracle/decks/trecon_small/config.h) built
    against the HIP host where the reference tree is.  4 plasma species at vth = 0.6 c, every particle with a tracer
    copy that the deck pushes itself, conducting walls, cleaning, strided field / hydro dumps with energy spectra
    appended, particle dumps.  The deck draws its normals from maxwellian_rand, which here is not the reference's
    ziggurat: the comparison is statistical.  The reference's own 1- and 2-rank runs (different seeds per rank)
    differ by up to 6 % in momentum moments and 7 % in E-field sums; bounds are about twice that."""
    exe = os.path.join(ROOT, "oracle", "_ref", "trecon%d.hip.exe" % nranks)
    mpiexec = "/opt/conda/bin/mpiexec"
    if not os.path.exists(exe) or (nranks > 1 and not os.path.exists(mpiexec)):
        pytest.skip("built where /root/reference is (python -c 'import __graft_entry__ as g; g.build()')")
    importlib.import_module("old-vpic_amd").lib()
    launch = [mpiexec, "-n", str(nranks)] if nranks > 1 else []
    run_deck(launch + [exe, "-tpp=1"], cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    sys.path.insert(0, ROOT)
    from oracle import trecon as T
    got = T.summarize(str(tmp_path), nranks)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "trecon.npz"))
    G = lambda k: gold["n%d_%s" % (nranks, k)]
    for name in ("info", "global.vpc", "rundata/species", "rundata/materials"):
        assert np.array_equal(got["file_" + name], G("file_" + name)), name
    total = 0
    for sp in T.SPECIES:
        total += int(got[sp + "_np"])
        assert abs(int(got[sp + "_np"]) - int(G(sp + "_np"))) <= 0.01 * int(G(sp + "_np")), sp      # which side of the sheet a particle is loaded on
        np.testing.assert_allclose(got[sp + "_u2"], G(sp + "_u2"), rtol=0.12, err_msg=sp)
        assert abs(got[sp + "_q"] / G(sp + "_q") - 1) <= 0.01, sp
        assert int(got[sp + "_hydro_bytes"]) == int(G(sp + "_hydro_bytes")), sp                     # header + 4 bands + energy.cxx's 6 appended blocks
        np.testing.assert_allclose(got[sp + "_hydro_sum"][3], G(sp + "_hydro_sum")[3], rtol=0.01, err_msg=sp)   # charge density
        a, b = got[sp + "_spectrum"], G(sp + "_spectrum")
        assert abs(a.sum() / b.sum() - 1) <= 0.01 and np.abs(np.cumsum(a) / a.sum() - np.cumsum(b) / b.sum()).max() <= 0.02, sp
    assert total == sum(int(G(sp + "_np")) for sp in T.SPECIES)                                     # nothing lost
    f, fr = got["field_sq_sum"], G("field_sq_sum")
    np.testing.assert_allclose(f[3:], fr[3:], rtol=2e-3)                                            # B: the sheet's own field
    np.testing.assert_allclose(f[:3], fr[:3], rtol=0.2)                                             # E: driven by the noise of the load


@pytest.mark.parametrize("nranks", [1, 2])
def test_production_reconnection_deck_with_the_references_normals(tmp_path, nranks):
    """The same production deck (16 x 4 x 8 cells: oracle/trecon.py --tiny) loading the REFERENCE's particles: the
    fixture carries every normal the reference run drew (recorded through its public mtrand API by
    oracle/normals_shim.c) and the HIP host replays them (VPIC_HIP_NORMALS), so both runs start from the same
    particles bit for bit and the comparison is held tighter than the hand-written sheet deck's: particle counts and
    charge exact, momentum moments 1e-5, charge density 1e-6, B-field sums 1e-6, E-field sums 1e-4, spectra 1e-3 after
    40 steps of a vth = 0.6 c plasma (measured: 8e-7, 4e-8, 1e-7, 6e-6, 8e-5)."""
    exe = os.path.join(ROOT, "oracle", "_ref", "trecontiny%d.hip.exe" % nranks)
    mpiexec = "/opt/conda/bin/mpiexec"
    if not os.path.exists(exe) or (nranks > 1 and not os.path.exists(mpiexec)):
        pytest.skip("built where /root/reference is (python -c 'import __graft_entry__ as g; g.build()')")
    importlib.import_module("old-vpic_amd").lib()
    sys.path.insert(0, ROOT)
    from oracle import trecon as T
    gold = np.load(os.path.join(ROOT, "tests", "golden", "trecon_tiny.npz"))
    G = lambda k: gold["n%d_%s" % (nranks, k)]
    for r in range(nranks):
        T.write_normals(str(tmp_path / ("normals.%d" % r)), G("normals_%d" % r), G("words_%d" % r))
    launch = [mpiexec, "-n", str(nranks)] if nranks > 1 else []
    env = dict(os.environ, VPIC_HIP_NORMALS=str(tmp_path / "normals"))
    run_deck(launch + [exe, "-tpp=1"], cwd=tmp_path, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    got = T.summarize(str(tmp_path), nranks, T.TINY)
    for name in ("info", "global.vpc", "rundata/species", "rundata/materials"):
        assert np.array_equal(got["file_" + name], G("file_" + name)), name
    worst = {}
    for sp in T.SPECIES:
        assert int(got[sp + "_np"]) == int(G(sp + "_np")), sp
        worst["u2"] = max(worst.get("u2", 0), np.abs(got[sp + "_u2"] / G(sp + "_u2") - 1).max())
        worst["q"] = max(worst.get("q", 0), abs(got[sp + "_q"] / G(sp + "_q") - 1))
        worst["rho"] = max(worst.get("rho", 0), abs(got[sp + "_hydro_sum"][3] / G(sp + "_hydro_sum")[3] - 1))
        a, b = got[sp + "_spectrum"], G(sp + "_spectrum")
        worst["spectrum"] = max(worst.get("spectrum", 0), np.abs(np.cumsum(a) / a.sum() - np.cumsum(b) / b.sum()).max())
        assert int(got[sp + "_hydro_bytes"]) == int(G(sp + "_hydro_bytes")), sp
    f, fr = got["field_sq_sum"], G("field_sq_sum")
    worst["B"] = np.abs(f[3:] / fr[3:] - 1).max()
    worst["E"] = np.abs(f[:3] / fr[:3] - 1).max()
    print("worst relative deviations from the reference run:", {k: float(v) for k, v in worst.items()})
    assert worst["u2"] <= 1e-5 and worst["q"] <= 1e-7 and worst["rho"] <= 1e-6, worst
    assert worst["B"] <= 1e-6 and worst["E"] <= 1e-4 and worst["spectrum"] <= 1e-3, worst
