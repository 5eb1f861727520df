"""serl_td3_train_wide -- the chunks of a minibatch of up to 512 rows on workgroups of their own: every array it writes against
serl_td3_train_big bit for bit (13 - 15 updates, so that every workgroup re-reads weight and partial lines it already holds), one chunk
against the kernels that generalises, split calls, two learners, a NaN-filled workspace, the refusals, and TD3.train(chunks='parallel').
There is no test of the time-out path: it would mean making workgroups wait on purpose."""
import ctypes
import random
import numpy as np
import pytest
import torch
import td3_64 as T
import td3_big as TB
import test_gpu_td3 as G
import test_gpu_td3_rng as R
import test_gpu_td3_big as GB

pytestmark = pytest.mark.gpu
OUT = GB.OUT


class Launch(GB.Launch):
    """test_gpu_td3_big.Launch with the workspace of serl_td3_wide_work_bytes (NaN-filled, the synchronisation block included) and a
    status array of -7 with a guard entry on either side"""

    def __init__(self, engine, cases, **kw):
        super().__init__(engine, cases, **kw)
        d0 = cases[0]
        self.big_wb = self.wb
        self.wb = int(self.L.serl_td3_wide_work_bytes(self.K, d0['S'], d0['A'], d0['H'], d0['L'], d0['B']))
        assert self.wb > self.big_wb and self.wb % 16 == 0
        self.work = torch.full((self.wb // 4 + 8,), float('nan'), dtype=torch.float32, device=self.dev)
        self.status = torch.full((self.K + 2,), -7, dtype=torch.int32, device=self.dev)

    def big_desc(self, **kw):
        """the descriptor of a serl_td3_train_big call on the same buffers"""
        d = self.desc(**kw)
        d.work_bytes = self.big_wb
        return d

    def run(self, entry='wide', dense=0, gen=False, learner0=0, first=0, **kw):
        if entry == 'old':
            return super().run('old', dense, gen, learner0, first=first, **kw)
        rd = self.rng_desc(dense, learner0) if gen else None
        if entry == 'big':
            d = self.big_desc(no_tables=gen, first=first, **kw)
            bd = self.C.Td3BigDesc(rng=ctypes.pointer(rd) if gen else None, dense=dense)
            rc = self.L.serl_td3_train_big(self.engine.ctx, ctypes.byref(d), ctypes.byref(bd), self.stream())
        else:
            d = self.desc(no_tables=gen, first=first, **kw)
            wd = self.C.Td3WideDesc(rng=ctypes.pointer(rd) if gen else None, status=self.status[1 + first].data_ptr(), dense=dense)
            rc = self.L.serl_td3_train_wide(self.engine.ctx, ctypes.byref(d), ctypes.byref(wd), self.stream())
        torch.cuda.synchronize()
        return rc

    def ran(self, first=0, K=None):
        K = self.K if K is None else K
        want = [-7] * (self.K + 2)
        want[1 + first:1 + first + K] = [0] * K
        return self.status.cpu().tolist() == want


def _same(a, b, what=''):
    for k in OUT:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s %s' % (what, k))


# ---- 1. every written array equals serl_td3_train_big ---------------------------------------------------------------------------------
@pytest.mark.parametrize('gen', [False, True], ids=['tables', 'rng'])
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
@pytest.mark.parametrize('c', TB.CASES, ids=T.case_id)
def test_wide_equals_big(engine, c, dense, gen):
    """the eight rows, adam_steps, td_loss, pg_loss, guard rows and spare columns: serl_td3_train_wide's are serl_td3_train_big's"""
    d, _ = GB._big(c)
    big, wide = Launch(engine, [d]), Launch(engine, [d])
    assert big.run('big', dense, gen, learner0=3) == 0, big.L.serl_last_error()
    assert wide.run('wide', dense, gen, learner0=3) == 0, wide.L.serl_last_error()
    assert wide.ran()
    a, b = big.out(), wide.out()
    wide.assert_guards(b)
    np.testing.assert_array_equal(b['steps'][1], [d['n'], d['n_actor']])
    assert np.isfinite(wide.result(b, 0)['td']).all() and np.abs(b['actor'][1, :wide.Pa] - wide.host['actor'][1, :wide.Pa]).max() > 0
    _same(a, b, T.case_id(c))


# ---- 2. one chunk ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gen', [False, True], ids=['tables', 'rng'])
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
@pytest.mark.parametrize('c', GB.ONE_CHUNK, ids=T.case_id)
def test_one_chunk_equals_the_old_kernel(engine, c, dense, gen):
    """B = 1, 86, 128: one workgroup per learner that waits on nothing, bit for bit serl_td3_train / _mfma / _rng"""
    d = GB._small(c)
    assert d['B'] in (1, 86, 128)
    old, new = Launch(engine, [d]), Launch(engine, [d])
    assert old.run('old', dense, gen) == 0, old.L.serl_last_error()
    assert new.run('wide', dense, gen) == 0, new.L.serl_last_error()
    assert new.ran()
    b = new.out()
    new.assert_guards(b)
    _same(old.out(), b, T.case_id(c))


# ---- 3. split calls, no updates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gen', [False, True], ids=['tables', 'rng'])
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
def test_two_calls_equal_one_and_zero_updates(engine, dense, gen):
    c = TB.CASES[12]                        # B = 300
    d, _ = GB._big(c)
    one = Launch(engine, [d])
    assert one.run('wide', dense, gen) == 0
    n1 = 5
    k1 = sum(1 for u in range(n1) if (d['it0'] + u + 1) % d['freq'] == 0)
    two = Launch(engine, [d])
    assert two.run('wide', dense, gen, n=n1) == 0 and two.ran()
    assert two.run('wide', dense, gen, n=d['n'] - n1, it0=d['it0'] + n1, u0=n1, k0=k1) == 0 and two.ran()
    _same(one.out(), two.out())
    z = Launch(engine, [d])
    z.status.zero_()
    assert z.run('wide', dense, gen, n=0) == 0
    z.assert_untouched()
    assert z.status.cpu().tolist() == [0, 0, 0]


# ---- 4. two learners -------------------------------------------------------------------------------------------------------------------
def test_two_learners_equal_two_launches(engine):
    c = TB.CASES[9]                         # B = 257: 2 x 3 workgroups
    cases = [GB._big(c, seed)[0] for seed in (None, 31)]
    for gen in (False, True):
        both = Launch(engine, cases)
        assert both.run('wide', 1, gen, learner0=5) == 0 and both.ran()
        o = both.out()
        both.assert_guards(o)
        for i in (0, 1):
            solo = Launch(engine, cases)
            assert solo.run('wide', 1, gen, learner0=5 + i, first=i, K=1) == 0 and solo.ran(i, 1)
            s = solo.out()
            for k in OUT:
                np.testing.assert_array_equal(s[k][1 + i], o[k][1 + i], err_msg='%s learner %d' % (k, i))
                np.testing.assert_array_equal(s[k][2 - i], solo.host[k][2 - i], err_msg=k)
        assert (o['critic'][1] != o['critic'][2]).any()


# ---- 5. what the workspace holds before the call does not matter ----------------------------------------------------------------------
def test_workspace_contents_do_not_matter(engine):
    """every launch above starts from a workspace of NaN, synchronisation block included; here from other bit patterns too"""
    d, _ = GB._big(TB.CASES[15])            # B = 512
    ref = Launch(engine, [d])
    assert ref.run('wide', 0) == 0 and ref.ran()
    for fill in (0.0, 1.0, -3.0e38):
        la = Launch(engine, [d])
        la.work[:-8] = fill
        assert la.run('wide', 0) == 0 and la.ran()
        _same(ref.out(), la.out(), 'fill %r' % fill)
    la = Launch(engine, [d])
    la.work[:-8].view(torch.int32).fill_(0x7FFFFFFF)
    assert la.run('wide', 0) == 0 and la.ran()
    _same(ref.out(), la.out(), 'fill all ones')


# ---- 6. refusals, each before any launch ---------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(engine):
    d, _ = GB._big(TB.CASES[6])             # B = 256
    la = Launch(engine, [d])
    C, L = la.C, la.L
    status = la.status[1].data_ptr()
    wide = lambda desc, wd: L.serl_td3_train_wide(engine.ctx, ctypes.byref(desc), ctypes.byref(wd) if wd is not None else None, la.stream())
    tables, rd = C.Td3WideDesc(rng=None, status=status, dense=0), la.rng_desc(0)
    gen = C.Td3WideDesc(rng=ctypes.pointer(rd), status=status, dense=0)
    assert wide(la.desc(), C.Td3WideDesc(rng=None, status=None, dense=0)) == C.E_INVALID
    assert wide(la.desc(), None) == C.E_INVALID
    assert wide(la.desc(), C.Td3WideDesc(rng=None, status=status, dense=2)) == C.E_INVALID
    for wd in (tables, gen):
        x = la.desc(); x.batch = 513; x.slot_cols = 600
        assert wide(x, wd) == C.E_UNSUPPORTED
        x = la.desc(); x.batch = 0
        assert wide(x, wd) == C.E_INVALID
        x = la.desc(); x.work_bytes = la.wb - 1
        assert wide(x, wd) == C.E_INVALID
        x = la.desc(); x.work_bytes = la.big_wb             # the chunked kernel's workspace is too small
        assert wide(x, wd) == C.E_INVALID
        for field, v in (('hidden', 132), ('num_layers', 5), ('state_dim', 17), ('action_dim', 5)):
            x = la.desc(); setattr(x, field, v)
            assert wide(x, wd) == C.E_UNSUPPORTED, field
        for field, v in (('actor', None), ('work', None), ('n_updates', -1), ('policy_update_freq', 0), ('capacity', 0), ('lr', 0.0)):
            x = la.desc(); setattr(x, field, v)
            assert wide(x, wd) == C.E_INVALID, field
        # more workgroups than CUs: n_learners x 2 chunks (nothing of the other learners is looked at before the refusal)
        cus = torch.cuda.get_device_properties(engine.device).multi_processor_count
        x = la.desc(); x.n_learners = cus // 2 + 1; x.work_bytes = 1 << 40
        assert wide(x, wd) == C.E_UNSUPPORTED
        assert 'CU' in L.serl_last_error().decode()
    x = la.desc(); x.slot_cols = d['B'] - 1
    assert wide(x, tables) == C.E_INVALID
    assert wide(la.desc(no_tables=True), C.Td3WideDesc(rng=ctypes.pointer(la.rng_desc(1)), status=status, dense=0)) == C.E_INVALID
    assert wide(la.desc(no_tables=True), tables) == C.E_INVALID
    bad = la.rng_desc(0); bad.n_rows = d['B'] - 1
    assert wide(la.desc(no_tables=True), C.Td3WideDesc(rng=ctypes.pointer(bad), status=status, dense=0)) == C.E_INVALID
    torch.cuda.synchronize()
    la.assert_untouched()
    assert la.status.cpu().tolist() == [-7, -7, -7]


# ---- 7. through TD3.train ---------------------------------------------------------------------------------------------------------
def test_td3_train_chunks_parallel(engine):
    """batch_size 256: chunks='parallel' ends where fused=True ends (modules and optimiser state), in every dense / draws combination,
    and says what it ran; the default call still reports 'eager'"""
    import serl_amd
    dev = engine.device
    S, A, H, Lh, B, n, it0, rows = 7, 3, 72, 3, 256, 13, 3, 600
    d0, _ = GB._big(TB.CASES[6])
    ring_rows = torch.from_numpy(d0['ring'][:rows])

    def learner():
        torch.manual_seed(5)
        t = serl_amd.TD3(G._args(S, A, H, Lh, 'tanh', B, 'cpu'), engine)
        ring = serl_amd.DeviceReplay(700, dev, engine, S, A)
        ring.append_rows(ring_rows)
        return t, ring

    t, ring = learner()
    assert t.fused_wide_supported(dev) and t.fused_big_supported(dev)
    t.train(ring, 2, iteration0=0, rng=random.Random(1), generator=torch.Generator().manual_seed(1))
    assert t.last_path == 'eager'
    for kw, path in ((dict(), 'fused-wide'), (dict(dense='mfma'), 'fused-mfma-wide'), (dict(draws='device', seed=77, learner=2), 'fused-wide-rng'),
                     (dict(draws='device', seed=77, learner=2, dense='mfma'), 'fused-mfma-wide-rng')):
        res = {}
        for chunks in ('serial', 'parallel'):
            t, ring = learner()
            out = t.train(ring, n, iteration0=it0, rng=random.Random(3), generator=torch.Generator().manual_seed(9), fused=True, chunks=chunks, **kw)
            res[chunks] = (R._state(t), out)
            assert t.last_path == (path if chunks == 'parallel' else path.replace('wide', 'big')), (t.last_path, kw)
        for k in res['serial'][0]:
            np.testing.assert_array_equal(res['serial'][0][k], res['parallel'][0][k], err_msg='%s %s' % (k, kw))
        assert res['serial'][1] == res['parallel'][1]
    # a minibatch of one chunk takes the wide entry too
    t = serl_amd.TD3(G._args(S, A, H, Lh, 'tanh', 86, 'cpu'), engine)
    t.train(ring, 3, iteration0=0, rng=random.Random(3), generator=torch.Generator().manual_seed(9), chunks='parallel')
    assert t.last_path == 'fused-wide'
