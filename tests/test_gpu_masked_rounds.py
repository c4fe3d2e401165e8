"""Masked passes over lists of more than 1024 tiles. The frame is 528 x 260: 33 x 65 = 2145 blocks, so
active_list_kernel takes three rounds of 1024 tiles and carries its base across them; with
CRT_PARTIAL_MB=2 the frame is two bands of 33 x 41 and 33 x 24 tiles (two rounds, then a band that
starts at a non-zero row). The caller sets the block words: in the active blocks sums, noise state
and preview equal crt_render_pass_async's bit for bit, the others are zeroed by the first pass and
left alone by the second. Before every masked pass a plain pass with another base seed runs over the
same frame, so the pass scratch (which the library's pool hands out again) never holds the
expected partial sums of a tile the list might have dropped."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H = 528, 260
BW, BH = 16, 4
NBX, NBY = W // BW, H // BH
NB = NBX * NBY
SPP, DEPTH = 8, 8
BOUNDS = [(0, 4), (4, 8)]
STOPPED = 0x80000000
NAN = float("nan")
PAD = 256        # doubles past the end of every output buffer
MARK = 7.25      # written into the skipped blocks between the passes: the second pass must not touch it


def pattern(name):
    """The active blocks (bool, NB) of a pattern."""
    on = np.zeros(NB, bool)
    if name == "all":
        on[:] = True
    elif name == "edges_of_rounds":
        on[[0, 1023, 1024, 1025, 2047, 2048, 2144]] = True
    elif name == "round2_stopped":
        on[:] = True
        on[1024:2048] = False
    elif name == "round1_stopped":
        on[1024:] = True
    elif name == "random_half":
        on[:] = np.random.default_rng(5).random(NB) < 0.5
    elif name != "none":
        raise ValueError(name)
    return on


PATTERNS = ["all", "edges_of_rounds", "round2_stopped", "round1_stopped", "random_half", "none"]


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def pixel_mask(on):
    import torch
    m = np.repeat(np.repeat(on.reshape(NBY, NBX), BH, axis=0), BW, axis=1)
    return torch.from_numpy(m).cuda()


def block_any(a):
    """(H, W, k) bool tensor -> per block: any pixel set (numpy, NB)."""
    return a.reshape(NBY, BH, NBX, BW, -1).permute(0, 2, 1, 3, 4).reshape(NB, -1).any(1).cpu().numpy()


class Job:
    """A scene at 528 x 260, 8 spp, depth 8: the plain passes' snapshots (the expected values), each
    pass's own partial sums, and the scrub pass; rendered once and left unchanged."""

    def __init__(self, crt, name, seed):
        import torch
        from cpp_raytracer_amd import camera_with
        d = crt.SceneData.named(name, seed)
        d.camera = camera_with(d.camera, image_w=W, image_h=H, samples_per_pixel=SPP, max_depth=DEPTH)
        self.s = crt.GpuScene(d)
        self.s.upload(0)
        self.cam = crt.resolve_camera(d.camera, 13)
        # the scrub's camera: another base seed, and also another background colour and the frame
        # upside down, since a block that sees only the background, only black or only a light holds
        # the same sums under every seed
        other = camera_with(d.camera)
        for k in range(3):
            other.background[k] = 0.5 * d.camera.background[k] + 0.25
            other.up[k] = -d.camera.up[k]
        self.scrub_cam = crt.resolve_camera(other, 977)
        assert crt.sample_chunk_len(SPP) == 4 and crt.block_count(W, H) == NB
        total, nz, out = (torch.full((H, W, k), NAN, dtype=torch.float64, device="cuda") for k in (3, 2, 3))
        self.snap, self.partial = {}, {}
        for a, b in BOUNDS:
            self.s.render_pass(0, self.cam, a, b - a, total.data_ptr(), nz.data_ptr(), out.data_ptr(), stream())
            self.snap[b] = (total.clone(), nz.clone(), out.clone())
            # the pass's own chunk sums, as its scratch holds them: the pass into a zeroed sum (0 + x = x)
            part = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
            self.s.render_pass(0, self.cam, a, b - a, part.data_ptr(), 0, 0, stream())
            self.partial[b] = part
        self.trash = [torch.full((H, W, k), NAN, dtype=torch.float64, device="cuda") for k in (3, 2, 3)]
        self.scrub()
        torch.cuda.synchronize()
        self.scrub_sum = self.trash[0].clone()
        assert all(torch.isfinite(t).all() for b in self.snap for t in self.snap[b])

    def scrub(self):
        """A plain pass of the same frame, chunk count and scene with another base seed (and
        background, upside down) into throw-away buffers: whatever a masked pass finds in its scratch afterwards
        is not its own."""
        t = self.trash
        self.s.render_pass(0, self.scrub_cam, 0, 4, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), stream())


@pytest.fixture(scope="module")
def rtow(crt):
    return Job(crt, "rtow_final", 42)   # LDS scene: one queue


@pytest.fixture(scope="module")
def tree(crt):
    return Job(crt, "christmas_tree", None)  # HBM scene: the draw over 8 segments


@pytest.fixture(params=["rtow", "tree"])
def job(request):
    return request.getfixturevalue(request.param)


def masked(crt, job, on, hint):
    """The two masked passes over caller-set words, checked after each; returns the final device
    buffers (sums, noise, preview) and words."""
    import torch
    n = H * W
    bufs = [torch.full((n * k + PAD,), NAN, dtype=torch.float64, device="cuda") for k in (3, 2, 3)]
    for b in bufs:
        b[-PAD:] = 123.0
    total, nz, out = (b[:-PAD].view(H, W, k) for b, k in zip(bufs, (3, 2, 3)))
    words0 = np.where(on, 0, STOPPED).astype(np.uint32)
    blocks = torch.from_numpy(np.concatenate([words0, np.zeros(PAD, np.uint32)]).view(np.int32).copy()).cuda()
    inside = pixel_mask(on)
    n_on = int(on.sum())
    for a, b in BOUNDS:
        job.scrub()
        job.s.render_pass_masked(0, job.cam, a, b - a, total.data_ptr(), nz.data_ptr(), out.data_ptr(), blocks.data_ptr(),
                                 hint, stream())
        # a rule that never stops a block (min_samples = the job's samples): the count of active blocks
        active = crt.adaptive_update(0, job.cam, nz.data_ptr(), blocks.data_ptr(), b, 1e9, SPP, stream())
        torch.cuda.synchronize()
        words = blocks.cpu().numpy().view(np.uint32)
        assert active == n_on
        assert (words[:NB][on] == b).all() and (words[:NB][~on] == STOPPED).all() and (words[NB:] == 0).all()
        for got, want in zip((total, nz, out), job.snap[b]):
            assert torch.equal(got[inside], want[inside]), (a, b)
        if a == 0:   # skipped blocks: zeroed by the pass from sample 0 ...
            assert all((t[~inside] == 0).all() for t in (total, nz, out))
            total[~inside] = MARK
            nz[~inside] = MARK
            out[~inside] = NAN
        else:        # ... and left alone by a later one, whose preview of a block without samples is 0
            assert (total[~inside] == MARK).all() and (nz[~inside] == MARK).all() and (out[~inside] == 0).all()
        assert all((b_[-PAD:] == 123.0).all() for b_ in bufs)
    return total, nz, out, words[:NB]


def test_the_scrub_differs_from_the_expected_sums_in_every_block(job):
    """What the scrub leaves in the pass scratch is no masked pass's expected partial sums, in any
    block (the all-black ones included, thanks to the scrub's background): a tile the list dropped
    cannot pass on stale scratch. (Another base seed alone leaves 484 background-only blocks of
    rtow_final and the blocks inside a light of christmas_tree with equal sums.)"""
    import torch
    for b in (4, 8):
        black = ~block_any(job.partial[b] != 0)
        differs = block_any(job.scrub_sum != job.partial[b])
        pixels = int((job.scrub_sum != job.partial[b]).any(-1).sum())
        print(f"pass ending at {b}: {int(black.sum())} all-black blocks of {NB}, the scrub differs in {int(differs.sum())} "
              f"blocks and {pixels} of {W * H} pixels")
        assert differs[~black].all() and differs.all() and (~black).sum() > NB // 5
    assert not torch.equal(job.snap[4][0], job.snap[8][0])


@pytest.mark.parametrize("name", PATTERNS)
def test_masked_passes_over_three_list_rounds(crt, job, name):
    import torch
    on = pattern(name)
    assert {"all": NB, "edges_of_rounds": 7, "round2_stopped": NB - 1024, "round1_stopped": NB - 1024, "none": 0}.get(
        name, int(on.sum())) == int(on.sum())
    first = masked(crt, job, on, 0)
    again = masked(crt, job, on, 10 ** 9)  # the hint sizes the grid only
    for a, b in zip(first[:3], again[:3]):
        assert torch.equal(a, b)
    assert np.array_equal(first[3], again[3])
    print(f"{name}: {int(on.sum())} of {NB} blocks active, rounds hold {[int(on[r:r + 1024].sum()) for r in (0, 1024, 2048)]}")


@pytest.mark.parametrize("name", ["random_half", "edges_of_rounds"])
def test_two_bands_give_the_same_bits(crt, monkeypatch, job, name):
    """One chunk of the frame's partial sums is 3.3 MB: a 2 MB budget makes two bands, of 41 and 24
    tile rows (1353 tiles: two list rounds; 792 tiles starting at owned row 164)."""
    import torch
    on = pattern(name)
    want = masked(crt, job, on, 0)
    monkeypatch.setenv("CRT_PARTIAL_MB", "2")
    got = masked(crt, job, on, 0)
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b)
    assert np.array_equal(got[3], want[3])
