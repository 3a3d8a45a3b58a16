"""GPU tests of the argument checks that micf_patch_sample and micf_patch_sample_warped share, at the C level: both entries are
called directly through the bound library, with a NULL map and field unless a case says otherwise, and must return the same code.

Every case passes real device memory and has exactly one faulty argument; every output buffer and the index buffer carry at least
64 bytes of slack beyond their nominal size, so a check that wrongly passed would launch on valid memory."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, -1, -2                  # include/micformer_hip.h
SLACK = 256
SHAPE, BIG = (12, 20, 24), (2049, 2, 2)              # BIG: an extent above the 2048 the kernels take
PATCH16, PATCH12 = (8, 8, 16), (8, 8, 12)


def _scan(shape, seed):
    from micformer_amd import patches
    g = torch.Generator().manual_seed(seed)
    values = torch.tensor((0,) + tuple(patches.MMWHS_LABEL_VALUES), dtype=torch.int16)
    ct = torch.randint(-1000, 2000, shape, generator=g, dtype=torch.int16)
    mr = torch.randint(0, 1500, shape, generator=g, dtype=torch.int16)
    lab = values[torch.randint(0, len(values), shape, generator=g)]
    return ct.cuda(), mr.cuda(), lab.cuda()


class _Setup:
    """The good arguments of a call for one patch size, as a dict; call(entry, **changes) makes the call with some replaced."""

    def __init__(self):
        from micformer_amd import _lib, loader, patches
        self.values = tuple(patches.MMWHS_LABEL_VALUES)
        self.scan = _scan(SHAPE, 5)
        built = patches.index_scans([self.scan])[0].buffer
        self.index_bytes = built.numel()
        self.index = torch.zeros(self.index_bytes + SLACK, dtype=torch.uint8, device="cuda")
        self.index[:self.index_bytes] = built
        self.big = _scan(BIG, 6)
        self.big_bytes = _lib.query_bytes("micf_patch_index_bytes", BIG[0] * BIG[1] * BIG[2], len(self.values), 1)
        self.big_index = torch.zeros(self.big_bytes + SLACK, dtype=torch.uint8, device="cuda")
        self.draws = patches.draw_patches(1, oversample_foreground_percent=1.0, generator=torch.Generator().manual_seed(7), device="cuda")
        self.field = torch.zeros((1, 3, 513, 2, 2), dtype=torch.float32, device="cuda")
        self.samples = {False: self._samples(loader, self.scan), True: self._samples(loader, self.big)}

    @staticmethod
    def _samples(loader, scan):
        items = (loader.LoaderSample * 1)()
        ct, mr, lab = scan
        it = items[0]
        it.ct, it.mr, it.label = ct.data_ptr(), mr.data_ptr(), lab.data_ptr()
        it.ct_shape[:], it.mr_shape[:], it.label_shape[:] = ct.shape, mr.shape, lab.shape
        it.ct_dtype, it.mr_dtype, it.label_dtype = (loader._IMAGE_DTYPES[ct.dtype], loader._IMAGE_DTYPES[mr.dtype],
                                                    loader._LABEL_DTYPES[lab.dtype])
        return items

    def outputs(self, patch):
        V = patch[0] * patch[1] * patch[2]
        return dict(image=torch.zeros(4 * V + SLACK, dtype=torch.uint8, device="cuda"),
                    label_map=torch.zeros(V + SLACK, dtype=torch.uint8, device="cuda"),
                    origins=torch.zeros(12 + SLACK, dtype=torch.uint8, device="cuda"),
                    picked=torch.zeros(16 + SLACK, dtype=torch.uint8, device="cuda"))

    def call(self, entry, patch, out, big=False, values=None, index_bytes=None, index_off=0, pad_class=0, clamp=0, padding_mode=0,
             image_off=0, label_off=0, picked_off=0, field=False, grid=(0, 0, 0)):
        """-> the entry's return code.  Every keyword is one argument of the C call, the defaults the good ones."""
        from micformer_amd import _lib, patch_warp, patches
        values = self.values if values is None else values
        vals = (ctypes.c_int32 * len(values))(*values)
        index = self.big_index if big else self.index
        ptrs = (ctypes.c_void_p * 1)(index.data_ptr() + index_off)
        sizes = (ctypes.c_int64 * 1)((self.big_bytes if big else self.index_bytes) if index_bytes is None else index_bytes)
        args = [ctypes.addressof(self.samples[big]), 1, ctypes.addressof(ptrs), ctypes.addressof(sizes), ctypes.addressof(vals),
                len(values), self.draws.data_ptr(), patch[0], patch[1], patch[2], padding_mode, pad_class, clamp,
                out["image"].data_ptr() + image_off, out["label_map"].data_ptr() + label_off, out["origins"].data_ptr(),
                out["picked"].data_ptr() + picked_off]
        with torch.cuda.device(0):
            if entry == "plain":
                rc = patches.lib.micf_patch_sample(*args, _lib.stream())
            else:
                rc = patch_warp.lib.micf_patch_sample_warped(*args, None, 0, self.field.data_ptr() if field else None, *grid, 0,
                                                             _lib.stream())
        torch.cuda.synchronize()
        return rc


@pytest.fixture(scope="module")
def setup():
    return _Setup()


ENTRIES = ("plain", "warped")

EINVAL_CASES = {
    "image + 2": dict(image_off=2),
    "label_map + 4": dict(label_off=4),
    "picked + 2": dict(picked_off=2),
    "pad_class 256": dict(pad_class=256),
    "clamp 2": dict(clamp=2),
    "padding_mode 2": dict(padding_mode=2),
    "a label value 0": dict(values=(205, 0, 420)),
    "duplicate label values": dict(values=(205, 420, 205)),
    "index_bytes one byte short": dict(index_bytes=-1),
    "index pointer off by 128": dict(index_off=128),
}


def test_the_good_calls_pass(setup):
    for patch in (PATCH16, PATCH12):
        out = setup.outputs(patch)
        assert [setup.call(e, patch, out) for e in ENTRIES] == [OK, OK], patch


@pytest.mark.parametrize("name", list(EINVAL_CASES), ids=lambda n: n.replace(" ", "_"))
def test_one_bad_argument_is_einval_from_both_entries(setup, name):
    change = dict(EINVAL_CASES[name])
    if change.get("index_bytes") == -1:
        change["index_bytes"] = setup.index_bytes - 1
    out = setup.outputs(PATCH16)
    codes = [setup.call(e, PATCH16, out, **change) for e in ENTRIES]
    assert codes == [EINVAL, EINVAL], (name, codes)


def test_an_extent_above_2048_is_eunsupported_and_einval_beats_it(setup):
    out = setup.outputs(PATCH16)
    assert [setup.call(e, PATCH16, out, big=True) for e in ENTRIES] == [EUNSUPPORTED, EUNSUPPORTED]
    assert [setup.call(e, PATCH16, out, big=True, pad_class=256) for e in ENTRIES] == [EINVAL, EINVAL]


def test_the_warped_entrys_own_grid_checks_keep_their_order(setup):
    out = setup.outputs(PATCH16)
    assert setup.call("warped", PATCH16, out, big=True, field=True, grid=(1, 2, 2)) == EINVAL          # before the scan's EUNSUPPORTED
    assert setup.call("warped", PATCH16, out, field=True, grid=(513, 2, 2)) == EUNSUPPORTED
    assert setup.call("warped", PATCH16, out, field=True, grid=(512, 2, 2)) == OK


def test_alignment_follows_the_outputs_per_thread(setup):
    """Pw = 12: the warped entry stores 4 outputs per thread (image aligned to 8 bytes, label_map to 4), the plain one 1; both take
    image + 8 and label_map + 4, and write there what the aligned call writes."""
    V = PATCH12[0] * PATCH12[1] * PATCH12[2]
    for entry in ENTRIES:
        a, b = setup.outputs(PATCH12), setup.outputs(PATCH12)
        assert setup.call(entry, PATCH12, a) == OK
        assert setup.call(entry, PATCH12, b, image_off=8, label_off=4) == OK
        assert torch.equal(a["image"][:4 * V], b["image"][8:8 + 4 * V]), entry
        assert torch.equal(a["label_map"][:V], b["label_map"][4:4 + V]), entry
        assert torch.equal(a["origins"][:12], b["origins"][:12]) and torch.equal(a["picked"][:16], b["picked"][:16]), entry
        assert a["image"][:4 * V].view(torch.float16).float().abs().sum() > 0 and int(a["label_map"][:V].max()) > 0, entry
        assert not b["image"][:8].any() and not b["image"][8 + 4 * V:].any() and not b["label_map"][4 + V:].any(), entry
