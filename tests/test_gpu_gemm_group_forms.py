"""The kernel forms of the grouped hi/lo-split GEMM (csrc/gemm_group.hip) through comic_gemm_group_form:
1 = four waves in lockstep, 2 = loader + MFMA waves one workgroup per CU, 3 = loader + MFMA waves two workgroups per CU.

The two loader/MFMA forms run one workgroup barrier per k-tile in BOTH roles, with the k-tile count rounded up to the
prefetch depth (4 and 2): a count that the roles derive differently is a hang, so the groups below walk 1 ... 9 k-tiles
with partial last tiles through every residue of both depths, for the three operand layouts.  Every problem is held to
float64 numpy at 5e-5 of the max-norm (the bound of test_gemm_group_matches_numpy_and_is_reproducible: hi*hi + hi*lo +
lo*hi keeps 16 mantissa bits per operand), a second launch must repeat the first bit for bit, and the forms must agree
bit for bit: same split plan, same product order, same slice-ordered combine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from tests.gpu_util import DEV, assert_close, dev, lib, stream, sync

KEEP = 0.75
TOL = 5e-5
K_RESIDUES = (4, 20, 36, 64, 100, 132, 160, 200, 260, 288)
_SIZES = (1, 33, 130, 257)


def _pad4(n):
    return (n + 3) // 4 * 4


class _Group:
    """A group of problems on the device, with float64 references.  spec = (type, M, N, K, extras); extras: lda, ldb, ldc,
    bias, mask (= ld_mask), beta, ones.  Leading dimensions default to the next multiple of 4 (16-byte loadable rows)."""

    def __init__(self, specs, seed):
        rng = np.random.default_rng(seed)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        self.specs = specs
        self.probs = (L.GemmProb * len(specs))()
        self.keep, self.refs, self.outs = [], [], []
        for i, (ty, M, N, K, ex) in enumerate(specs):
            ones = ex.get('ones', False)
            lda = ex.get('lda', _pad4(M if ty == 0 else K))
            ldb = ex.get('ldb', _pad4(K if ty == 2 else N))
            ldc = ex.get('ldc', N)
            if ones:
                Am = np.ones((1, K), np.float32)
                dA = None
            else:
                Afull = f(K, lda) if ty == 0 else f(M, lda)
                Am = Afull[:, :M].T if ty == 0 else Afull[:, :K]
                dA = dev(Afull)
            Bfull = f(N, ldb) if ty == 2 else f(K, ldb)
            Bm = Bfull[:, :K].T if ty == 2 else Bfull[:, :N]
            ref = Am.astype(np.float64) @ Bm.astype(np.float64)
            C0 = f(M, ldc)
            bias = f(N) if ex.get('bias') else None
            if bias is not None:
                ref = ref + bias
            mask, ldm = None, 0
            if 'mask' in ex:
                ldm = ex['mask']
                mask = (rng.uniform(size=(M, ldm)) < KEEP).astype(np.float32)
                ref = ref / KEEP * mask[:, :N]
            beta = ex.get('beta', 0.0)
            ref = ref + beta * C0[:, :N]
            dB, dC = dev(Bfull), dev(C0)
            db = dev(bias) if bias is not None else None
            dm = dev(mask) if mask is not None else None
            self.keep += [dA, dB, db, dm]
            q = self.probs[i]
            q.A = dA.data_ptr() if dA is not None else None
            q.B, q.C = dB.data_ptr(), dC.data_ptr()
            q.bias = db.data_ptr() if db is not None else None
            q.mask = dm.data_ptr() if dm is not None else None
            q.M, q.N, q.K, q.lda, q.ldb, q.ldc, q.ld_mask = M, N, K, (1 if ones else lda), ldb, ldc, ldm
            q.alpha, q.beta, q.keep, q.type, q.ones_a = 1.0, beta, KEEP, ty, int(ones)
            self.refs.append(ref)
            self.outs.append((dC, C0, N))
        self.nbytes = int(lib().comic_gemm_group_workspace(self.probs, len(specs)))
        assert self.nbytes > 0
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=DEV)

    def launch(self, form):
        """Fresh outputs, one launch with `form`; returns (rc, [host copies of the C buffers])."""
        for dC, C0, _ in self.outs:
            dC.copy_(torch.from_numpy(C0))
        rc = lib().comic_gemm_group_form(self.probs, len(self.specs), self.ws.data_ptr(), self.nbytes, form, stream())
        sync()
        return rc, [dC.cpu().numpy() for dC, _, _ in self.outs]

    def check_forms(self, forms=(1, 2, 3)):
        """Every form: against float64 at TOL, nothing written outside the N columns, a second launch bit-equal; then the
        forms bit-equal to each other."""
        per_form = {}
        for form in forms:
            rc, got = self.launch(form)
            assert rc == 0, 'form %d: %s' % (form, lib().comic_last_error().decode())
            for g, (dC, C0, N), ref, sp in zip(got, self.outs, self.refs, self.specs):
                e = assert_close(g[:, :N], ref, TOL, 'form %d, problem %r' % (form, sp[:4]))
                print('form %d %r: rel err %.2e' % (form, sp[:4], e))
                assert np.array_equal(g[:, N:], C0[:, N:]), 'form %d wrote outside its columns (%r)' % (form, sp[:4])
            rc, again = self.launch(form)
            assert rc == 0
            for a, b, sp in zip(got, again, self.specs):
                assert np.array_equal(a, b), 'form %d: second launch differs (%r)' % (form, sp[:4])
            per_form[form] = got
        for form in forms[1:]:
            for a, b, sp in zip(per_form[forms[0]], per_form[form], self.specs):
                assert np.array_equal(a, b), 'forms %d and %d differ (%r)' % (forms[0], form, sp[:4])


@pytest.mark.parametrize('ty', [0, 1, 2], ids=['TN', 'NN', 'NT'])
def test_k_tile_residues(ty):
    """1 ... 9 k-tiles with partial last tiles: every residue of both prefetch depths; M, N in {1, 33, 130, 257} (one
    thread row, ragged tiles, more than one tile, one element past two tiles), and N = 258 in rows of 260."""
    specs = []
    for i, K in enumerate(K_RESIDUES):
        specs.append((ty, _SIZES[i % 4], _SIZES[(i + 1 + i // 4) % 4], K, {}))
    specs.append((ty, 130, 258, 100, {} if ty == 2 else {'ldb': 260}))
    if ty == 2:
        specs.append((ty, 33, 258, 260, {'ldc': 260}))
    assert {s[1] for s in specs} >= set(_SIZES) and {s[2] for s in specs} >= set(_SIZES)
    _Group(specs, 11 + ty).check_forms()


def test_split_tiles():
    """One TN problem 256 x 256 x 4096: four tiles, so the plan splits k and a slice starts at k > 0 on the
    row-contiguous operands; the partial tiles are combined inside the launch."""
    _Group([(0, 256, 256, 4096, {})], 21).check_forms()


def test_more_than_one_round():
    """Five TN problems 1024 x 1024 x 96: 320 work items -- more than the 256 resident workgroups of form 2, and a
    second workgroup on some CUs for forms 1 and 3 (512 slots)."""
    _Group([(0, 1024, 1024, 96, {})] * 5, 22).check_forms()


def test_epilogues_and_column_sums():
    """Bias, mask / keep and beta epilogues beside two column sums (ones_a) in one group: the column sums run in the
    same workgroups as the products, in every form with the same eight row groups."""
    specs = [
        (2, 64, 768, 2048, {'bias': True}),
        (1, 64, 768, 2048, {'mask': 768, 'ldc': 1280}),
        (2, 300, 256, 520, {'mask': 260, 'bias': True}),
        (0, 36, 72, 20, {'beta': 2.0}),
        (1, 132, 130, 44, {'bias': True, 'beta': -1.0}),
        (0, 1, 2048, 1920, {'ones': True}),
        (0, 1, 258, 1856, {'ones': True, 'ldb': 260}),
    ]
    _Group(specs, 23).check_forms()


def test_unaligned_rows_are_refused_by_the_loader_forms():
    """lda % 4 != 0: rows that cannot be loaded 16 bytes at a time.  Form 0 answers (with the four-wave kernel); forms 2
    and 3 return an error and launch nothing: the output buffers keep their contents."""
    g = _Group([(1, 70, 64, 45, {'lda': 45}), (0, 128, 128, 64, {})], 24)
    rc, got = g.launch(0)
    assert rc == 0, lib().comic_last_error().decode()
    for a, (dC, C0, N), ref in zip(got, g.outs, g.refs):
        assert_close(a[:, :N], ref, TOL, 'form 0 on unaligned rows')
    rc1, got1 = g.launch(1)
    assert rc1 == 0
    for a, b in zip(got, got1):
        assert np.array_equal(a, b)
    for form in (2, 3):
        rc, out = g.launch(form)
        assert rc != 0, 'form %d accepted rows of 45 floats' % form
        for a, (dC, C0, N) in zip(out, g.outs):
            assert np.array_equal(a, C0), 'form %d wrote although it refused the call' % form
    rc, _ = g.launch(4)
    assert rc != 0


def test_resident_workgroups_per_cu():
    assert lib().comic_gemm_group_resident(3) == 2
    assert lib().comic_gemm_group_resident(1) == 2
    assert lib().comic_gemm_group_resident(2) == 1
    assert lib().comic_gemm_group_resident(0) < 0
