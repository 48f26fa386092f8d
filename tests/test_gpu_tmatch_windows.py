"""gsh_match_template_windows_batch, gsh_locate_template_windows_batch and gsh_search_windows_batch on the MI355X: the cases
of tests/tmatch_window_cases.py on device memory with every wave of a launch in flight at once (the emulator runs one block
at a time, so only here do the 64-bit atomic maxima of a window's key word really race), a launch that fills the chip, and a
tracking chain locate -> search_windows -> locate ... enqueued on a caller's stream with no host sync between the calls."""
import numpy as np
import pytest

import tmatch_window_cases as tw
from parity_cases import Mem

pytestmark = pytest.mark.gpu
MEM = Mem("device")


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle import pyoracle
    return [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])


@pytest.mark.parametrize("case", tw.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_tmatch_windows_gpu(hip, oracles, case):
    case(hip, MEM, oracles)


def test_a_launch_that_fills_the_chip(hip, oracle):
    """10: eight frames of 320 x 180, 2048 windows of 48 x 48 at seeded places, a 16 x 16 template per window cut from inside
    it: 33 x 33 maps, four blocks a window, 8192 blocks of four waves, up to sixteen atomic maxima on one key word.  Every
    point is the place the template was cut from and every score 255; 64 seeded windows against the oracle, maps included."""
    import torch
    n, nwin, ws, t = 8, 2048, 48, 16
    img = tw.frames(71, n, 180, 320)
    rng = np.random.default_rng(72)
    windows = np.stack([rng.integers(0, 320 - ws + 1, nwin), rng.integers(0, 180 - ws + 1, nwin), np.full(nwin, ws), np.full(nwin, ws)], 1).astype(np.uint32)
    frame_of = rng.integers(0, n, nwin).astype(np.uint32)
    at = windows[:, :2] + rng.integers(0, ws - t + 1, (nwin, 2)).astype(np.uint32)
    tmpl = np.stack([img[f, y:y + t, x:x + t] for (x, y), f in zip(at, frame_of)])
    d_img, d_t = torch.from_numpy(np.array(img)).cuda(), torch.from_numpy(tmpl).cuda()
    d_win, d_fo = MEM.put(windows), MEM.put(frame_of)
    best = torch.full((nwin, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    score = torch.full((nwin,), tw.FILL, dtype=torch.uint8, device="cuda")
    hip.locate_template_windows_batch(d_img, d_t, d_win, (ws, ws), best, score, d_fo)
    some = np.sort(rng.choice(nwin, 64, replace=False))
    maps = torch.full((64, ws - t + 1, ws - t + 1), tw.FILL, dtype=torch.uint8, device="cuda")
    hip.match_template_windows_batch(maps, d_img, d_t[torch.from_numpy(some).cuda()].contiguous(), MEM.put(windows[some]), (ws, ws), MEM.put(frame_of[some]))
    torch.cuda.synchronize()
    b, s, m = best.cpu().numpy().view(np.uint32), score.cpu().numpy(), maps.cpu().numpy()
    assert np.array_equal(b, at), np.argwhere(b != at)[:4]
    assert (s == 255).all()
    for k, p in enumerate(some):
        x, y, w, h = (int(v) for v in windows[p])
        want = oracle.match_template(oracle.crop(img[frame_of[p]], x, y, w, h), tmpl[p])
        assert np.array_equal(m[k], want), "map of window %d: %d bytes differ" % (p, np.count_nonzero(m[k] != want))
        bx, by = oracle.find_best_match(want)
        assert (x + bx, y + by) == tuple(b[p]) and want[by, bx] == s[p]
    assert torch.equal(d_img.cpu(), torch.from_numpy(np.array(img))) and torch.equal(d_t.cpu(), torch.from_numpy(tmpl))
    assert np.array_equal(d_win.cpu().numpy().view(np.uint32), windows) and np.array_equal(d_fo.cpu().numpy().view(np.uint32), frame_of)


def test_tracking_chain_unsynced_on_a_caller_stream(hip, oracle):
    """11: a 16 x 16 patch moves by (+3, -2) a frame through five noise frames.  Step k locates it in frame k inside the windows
    of step k - 1 and search_windows (margin 6) makes the next windows of what it found -- after gsh_set_stream on a torch
    stream and under gsh_set_async(1) with nothing between the calls; compared after ONE sync with the run that synchronised
    after every call and with the oracle chain.  The second track starts on an invalid point and stays invalid."""
    import torch
    n, ih, iw, t, margin = 5, 120, 200, 16, 6
    img = np.array(tw.frames(73, n, ih, iw))
    patch = np.array(tw.frames(74, 1, t, t)[0])
    places = [(60 + 3 * k, 70 - 2 * k) for k in range(n)]
    for k, (x, y) in enumerate(places):
        img[k, y:y + t, x:x + t] = patch
    start = np.array([places[0], (tw.INVALID, tw.INVALID)], np.uint32)
    bound = (t + 2 * margin, t + 2 * margin)

    want, at = [], start  # the oracle chain
    for k in range(n):
        wins = tw.search_windows(at, t, t, margin, margin, iw, ih)
        step = tw.expected([oracle], ("chain", k), img, patch, wins, [k, k], bound)
        at = np.array([b for _, b, _ in step], np.uint32)
        want.append((wins, at, np.array([s for _, _, s in step], np.uint8)))
        assert tuple(at[0]) == places[k] and step[0][2] == 255 and tuple(at[1]) == (tw.INVALID, tw.INVALID) and not wins[1].any()

    def chain(sync):
        d_img, d_patch, d_at = torch.from_numpy(img).cuda(), torch.from_numpy(patch).cuda(), MEM.put(start)
        wins = torch.full((n, 2, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        best = torch.full((n, 2, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        score = torch.full((n, 2), tw.FILL, dtype=torch.uint8, device="cuda")
        frame_of = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(2).view(n, 2).contiguous()
        sync()
        for k in range(n):
            hip.search_windows_batch(d_at if k == 0 else best[k - 1], (t, t), (margin, margin), (iw, ih), wins[k]), sync()
            hip.locate_template_windows_batch(d_img, d_patch, wins[k], bound, best[k], score[k], frame_of[k]), sync()
        return wins, best, score

    synced = [a.cpu().numpy() for a in chain(torch.cuda.synchronize)]
    for k, (w, b, s) in enumerate(want):
        assert np.array_equal(synced[0][k].view(np.uint32), w) and np.array_equal(synced[1][k].view(np.uint32), b) and np.array_equal(synced[2][k], s), k
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        hip.set_stream(st.cuda_stream)
        hip.set_async(True)
        with torch.cuda.stream(st):
            out = chain(lambda: None)
        st.synchronize()
        got = [a.cpu().numpy() for a in out]
    finally:
        hip.set_async(False)
        hip.set_stream(None)
    for a, b in zip(got, synced):
        assert np.array_equal(a, b)
