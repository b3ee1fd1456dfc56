"""Engine: one libnestmc context = one GPU's shard of chains.

Python-facing arrays are chain-major ([C, P, G], [C, G], [C, P]) like the oracle;
the device keeps chain-fastest SoA ([P][G][C]) so each wavefront's 64 lanes (64
chains) touch consecutive addresses.  Conversions happen only at the boundary
(state upload, sample download), never inside the iteration loop.
"""

import ctypes

import numpy

from . import _lib
from . import priors as _priors
from ._lib import as_f64, check, dptr

# step-kernel modes reported by nmc_launch_config (step.h NMC_MODE_*)
MODE_NAMES = {0: "NMC_MODE_NOPOOL", 1: "NMC_MODE_LAUNCH", 2: "NMC_MODE_SYNC",
              3: "NMC_MODE_SYNC_LDS", 4: "NMC_MODE_SYNC_REG", 5: "NMC_MODE_SYNC_OWN",
              6: "NMC_MODE_HALF"}


class Engine:
    def __init__(self, family, sizes, n_chains, pooling, priors=None, *, seed=0,
                 chain_base=0, device=0, rng="philox"):
        lib = _lib.load()
        self.lib = lib
        self.family = family
        self.sizes = numpy.asarray(sizes, dtype=numpy.int64)
        self.off = numpy.ascontiguousarray(numpy.concatenate([[0], numpy.cumsum(self.sizes)]),
                                           dtype=numpy.int64)
        self.G = len(self.sizes)
        self.C = int(n_chains)
        self.P = int(family.n_params)
        self.pooling = pooling
        self.chain_base = int(chain_base)
        self.device = int(device)
        obs = as_f64(family.obs())
        if obs.shape[0] != self.off[-1]:
            raise ValueError("family has %d observations, groups sum to %d"
                             % (obs.shape[0], self.off[-1]))
        consts = as_f64(family.consts())
        if pooling == "partial":
            pfam, pprm = None, None
        else:
            if priors is None or len(priors) != self.P:
                raise ValueError("Invalid prior")
            pfam, pprm = _priors.encode_all(priors)
        h = ctypes.c_void_p()
        check(lib.nmc_create(
            ctypes.byref(h), self.device, self.C, self.chain_base, self.G, self.P,
            _lib.POOLING[pooling], family.family_id(), dptr(consts), len(consts),
            self.off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), dptr(obs),
            obs.shape[0], obs.shape[1],
            None if pfam is None else pfam.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
            None if pprm is None else dptr(pprm), ctypes.c_uint32(seed & 0xFFFFFFFF),
            _lib.RNG[rng]))
        self.h = h
        self._keep = (obs, consts, pfam, pprm)
        self.n_rows = 0
        self.cols = 0

    # -- lifecycle -----------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.nmc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- layout helpers -----------------------------------------------------
    @staticmethod
    def _pgc(a):          # [C, P, G] -> [P][G][C]
        return numpy.ascontiguousarray(numpy.transpose(numpy.asarray(a, float), (1, 2, 0)))

    @staticmethod
    def _gc(a):           # [C, G] -> [G][C]
        return numpy.ascontiguousarray(numpy.asarray(a, float).T)

    # -- state ----------------------------------------------------------------
    def set_state(self, value, log_prior, ll, mu=None, s2=None, scale=None):
        v = self._pgc(value)
        lp = self._pgc(log_prior)
        L = self._gc(ll)
        m = None if mu is None else self._gc(mu)        # [C, P] -> [P][C]
        s = None if s2 is None else self._gc(s2)
        sc = None if scale is None else self._pgc(scale)
        check(self.lib.nmc_set_state(self.h, dptr(v), dptr(lp), dptr(L), dptr(m), dptr(s),
                                     dptr(sc)))

    def get_state(self):
        C, P, G = self.C, self.P, self.G
        v = numpy.empty((P, G, C)); lp = numpy.empty((P, G, C)); L = numpy.empty((G, C))
        m = numpy.empty((P, C)); s = numpy.empty((P, C)); sc = numpy.empty((P, G, C))
        check(self.lib.nmc_get_state(self.h, dptr(v), dptr(lp), dptr(L), dptr(m), dptr(s),
                                     dptr(sc)))
        tr = lambda a: numpy.ascontiguousarray(numpy.transpose(a, (2, 0, 1)))   # noqa: E731
        return dict(value=tr(v), log_prior=tr(lp), ll=L.T.copy(), mu=m.T.copy(),
                    s2=s.T.copy(), scale=tr(sc))

    def log_prior(self):
        """[C, P, G]: the log priors as the reference holds them after the last iteration
        (nmc_get_log_prior) -- under partial pooling each value's normal log density under the
        current hyper-parameters, where get_state()["log_prior"] is the device's copy under
        the hyper-parameters of the step that decided the value."""
        lp = numpy.empty((self.P, self.G, self.C))
        check(self.lib.nmc_get_log_prior(self.h, dptr(lp)))
        return numpy.ascontiguousarray(numpy.transpose(lp, (2, 0, 1)))

    def set_replay(self, z, u, hz, hu):
        """z, u: [C, iter, P, G]; hz, hu: [C, iter, P] -> device [iter][P][G][C]."""
        zz = numpy.ascontiguousarray(numpy.transpose(z, (1, 2, 3, 0)), dtype=float)
        uu = numpy.ascontiguousarray(numpy.transpose(u, (1, 2, 3, 0)), dtype=float)
        hzz = numpy.ascontiguousarray(numpy.transpose(hz, (1, 2, 0)), dtype=float)
        huu = numpy.ascontiguousarray(numpy.transpose(hu, (1, 2, 0)), dtype=float)
        check(self.lib.nmc_set_replay(self.h, dptr(zz), dptr(uu), dptr(hzz), dptr(huu),
                                      zz.shape[0]))

    # -- schedule / run -------------------------------------------------------
    def set_schedule(self, n_iter, burn, thin, tune_interval=100):
        check(self.lib.nmc_set_schedule(self.h, n_iter, burn, thin, tune_interval))
        r, c = ctypes.c_int(), ctypes.c_int()
        check(self.lib.nmc_n_rows(self.h, ctypes.byref(r), ctypes.byref(c)))
        self.n_rows, self.cols = r.value, c.value

    def set_trace(self, enable=True):
        check(self.lib.nmc_set_trace(self.h, 1 if enable else 0))

    def run(self, iter_begin, iter_end):
        check(self.lib.nmc_run(self.h, iter_begin, iter_end))

    def synchronize(self):
        check(self.lib.nmc_synchronize(self.h))

    def prefill(self, i0, i1):
        """Draw the variates of iterations [i0, i1) now, beside whatever runs, for a later
        run() starting at i0 (nmc_prefill; run() guesses its next call by itself)."""
        check(self.lib.nmc_prefill(self.h, int(i0), int(i1)))

    def prefill_stats(self):
        """{"issued": iterations drawn by prefills, "used": iterations run() took from one}."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.nmc_prefill_stats(self.h, ctypes.byref(a), ctypes.byref(b)))
        return {"issued": a.value, "used": b.value}

    def set_resident(self, on=True):
        """One step launch for consecutive run() calls (nmc_set_resident): a call continuing
        the last is handed to the running launch.  Results are bit-identical either way."""
        check(self.lib.nmc_set_resident(self.h, 1 if on else 0))

    def resident_stats(self):
        """{"enabled", "active", "launches", "calls", "last_refusal"} (nmc_resident_stats)."""
        e, a, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        n, c = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.nmc_resident_stats(self.h, ctypes.byref(e), ctypes.byref(a),
                                          ctypes.byref(n), ctypes.byref(c), ctypes.byref(w)))
        return {"enabled": bool(e.value), "active": bool(a.value), "launches": n.value,
                "calls": c.value, "last_refusal": w.value}

    def variate_plan(self):
        """Verification hook: {"vcap": iterations one variate buffer holds, "chunk":
        iterations per step launch, "counter_wrap": the limit of set_counter_wrap,
        "counter_resets": resets so far} (nmc_debug_variate_plan, nmc_debug_counter_resets)."""
        v, c = ctypes.c_int(), ctypes.c_int()
        w, n = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.nmc_debug_variate_plan(self.h, ctypes.byref(v), ctypes.byref(c),
                                              ctypes.byref(w)))
        check(self.lib.nmc_debug_counter_resets(self.h, ctypes.byref(n)))
        return {"vcap": v.value, "chunk": c.value, "counter_wrap": w.value,
                "counter_resets": n.value}

    def set_counter_wrap(self, limit):
        """Verification hook (nmc_debug_set_counter_wrap): reset the counters that run on
        across launches before they would reach ``limit`` (1 .. 2**31, the default), so that
        a short run meets the reset.  No effect on results; no product path calls this."""
        check(self.lib.nmc_debug_set_counter_wrap(self.h, int(limit)))

    # -- results --------------------------------------------------------------
    def samples_raw(self, row_begin=0, n_rows=None):
        """[rows][cols][C] exactly as stored on the device."""
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        out = numpy.empty((n_rows, self.cols, self.C))
        check(self.lib.nmc_get_samples(self.h, row_begin, n_rows, dptr(out)))
        return out

    def set_samples_raw(self, x, row_begin=0):
        """Verification hook (nmc_debug_set_samples), the inverse of samples_raw: write
        x [rows][cols][C] (float64, C-contiguous) into the device sample store from row
        row_begin on.  The store is the one set_schedule sized; no product path calls this."""
        if not (isinstance(x, numpy.ndarray) and x.dtype == numpy.float64 and x.ndim == 3
                and x.shape[1:] == (self.cols, self.C) and x.flags["C_CONTIGUOUS"]):
            raise ValueError("x must be a C-contiguous float64 array [rows][%d][%d]"
                             % (self.cols, self.C))
        check(self.lib.nmc_debug_set_samples(self.h, int(row_begin), x.shape[0], dptr(x)))

    def samples(self):
        """[C, rows, cols] chain-major (the oracle's row layout)."""
        return numpy.ascontiguousarray(numpy.transpose(self.samples_raw(), (2, 0, 1)))

    def accept_counts(self):
        out = numpy.empty((self.P, self.G, self.C), dtype=numpy.int64)
        check(self.lib.nmc_get_accept_counts(self.h, out.ctypes.data_as(
            ctypes.POINTER(ctypes.c_int64))))
        return numpy.transpose(out, (2, 0, 1))

    def trace(self, n_iter):
        n = n_iter * self.P * self.G * self.C
        acc = numpy.empty(n, dtype=numpy.uint8)
        llp = numpy.empty(n)
        check(self.lib.nmc_get_trace(self.h, acc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                     dptr(llp)))
        sh = (n_iter, self.P, self.G, self.C)
        # -> [C, iter, P, G]
        return (numpy.transpose(acc.reshape(sh), (3, 0, 1, 2)),
                numpy.transpose(llp.reshape(sh), (3, 0, 1, 2)))

    def eval_group_ll(self, theta):
        """theta [C, P, G] -> group log-likelihoods [C, G] on the device."""
        th = self._pgc(theta)
        out = numpy.empty((self.G, self.C))
        check(self.lib.nmc_eval_group_ll(self.h, dptr(th), dptr(out)))
        return out.T.copy()

    def obs_ll_rows(self, row_begin=0, n_rows=None):
        """Per-observation LL at recorded rows of the sample store: [C, rows, n_obs]."""
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        out = numpy.empty((self.C, n_rows, int(self.off[-1])))
        check(self.lib.nmc_obs_ll_rows(self.h, row_begin, n_rows, dptr(out)))
        return out

    def write_ll_csvs(self, sample_dir, chain_ids, threads=8):
        """logLikelihood.<id>.csv for every local chain and recorded row (streamed)."""
        ids = numpy.ascontiguousarray(chain_ids, dtype=numpy.int32)
        if len(ids) != self.C:
            raise ValueError("need one file id per local chain")
        d = sample_dir if sample_dir.endswith("/") else sample_dir + "/"
        check(self.lib.nmc_write_ll_csvs(self.h, d.encode(),
                                         ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                         int(threads)))

    def waic_partials(self, row_begin=0, n_rows=None, n_valid=None):
        """WAIC's per-observation state (m, s, n, mean, M2) of every chain block over recorded
        rows [row_begin, row_begin + n_rows) and local chains [0, n_valid): [CB, 5, n_obs],
        reduced on the device from the sample store (nmc_waic_partials; nestmc.waic).  Chains
        from n_valid on (padding) enter as the identity.  A term that is not finite is an
        error."""
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        if n_valid is None:
            n_valid = self.C
        out = numpy.empty(((self.C + 63) // 64, 5, int(self.off[-1])))
        bad = ctypes.c_int64()
        check(self.lib.nmc_waic_partials(self.h, int(row_begin), int(n_rows), int(n_valid),
                                         dptr(out), ctypes.byref(bad)))
        self.waic_nonfinite = bad.value
        if bad.value:
            raise _lib.NestmcError("WAIC: %d per-observation log-likelihood terms were not "
                                   "finite" % bad.value)
        return out

    def waic(self, row_begin=0, n_rows=None, n_valid=None):
        """The WaicResult (nestmc.waic) of this engine's chains: its chain blocks' partials
        merged in chain-block order."""
        from . import waic as _waic
        parts = self.waic_partials(row_begin, n_rows, n_valid)
        return _waic.finish(_waic.merge(list(parts)), self.off)

    # -- posterior predictive checks (nestmc.ppc; csrc/ppc.h) -------------------------------
    def n_resp(self):
        """The response fields the family can draw replicates of (0: it cannot draw)."""
        n = ctypes.c_int()
        check(self.lib.nmc_ppc_nresp(self.h, ctypes.byref(n)))
        return n.value

    def observed(self):
        """y [n_obs, NRESP]: the family's table at its response fields."""
        return numpy.ascontiguousarray(self._keep[0][:, list(self.family.response_fields())])

    def predictive_draws(self, row_begin=0, n_rows=None):
        """The posterior predictive replicates at recorded rows of the sample store,
        [C, rows, n_obs, NRESP] (nmc_ppc_draws): for small windows, tests and statistics of
        one's own -- Engine.ppc never forms them."""
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        out = numpy.empty((self.C, max(int(n_rows), 0), int(self.off[-1]), max(self.n_resp(), 1)))
        check(self.lib.nmc_ppc_draws(self.h, int(row_begin), int(n_rows), dptr(out)))
        return out

    def ppc_partials_raw(self, row_begin=0, n_rows=None, n_valid=None):
        """nmc_ppc_partials as it answers: (the chain blocks' partials, a list of nestmc.ppc
        dicts in chain-block order, each with nonfinite = 0; the call's non-finite count)."""
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        if n_valid is None:
            n_valid = self.C
        CB, n, NR = (self.C + 63) // 64, int(self.off[-1]), max(self.n_resp(), 1)
        ost = numpy.empty((CB, 3, NR, n))
        oct_ = numpy.empty((CB, 2, NR, n), dtype=numpy.uint32)
        gst = numpy.empty((CB, self.G, NR, 4, 3))
        gct = numpy.empty((CB, self.G, NR, 4, 2), dtype=numpy.uint32)
        ty = numpy.empty((self.G, NR, 4))
        bad = ctypes.c_int64()
        u32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))   # noqa: E731
        check(self.lib.nmc_ppc_partials(self.h, int(row_begin), int(n_rows), int(n_valid),
                                        dptr(ost), u32(oct_), dptr(gst), u32(gct), dptr(ty),
                                        ctypes.byref(bad)))
        parts = [dict(obs_state=ost[b], obs_count=oct_[b].astype(numpy.int64),
                      group_state=gst[b], group_count=gct[b].astype(numpy.int64), ty=ty,
                      nonfinite=0) for b in range(CB)]
        return parts, bad.value

    def ppc_partials(self, row_begin=0, n_rows=None, n_valid=None):
        """The posterior predictive partials of every chain block over recorded rows
        [row_begin, row_begin + n_rows) and local chains [0, n_valid), reduced on the device
        from the sample store (nmc_ppc_partials; nestmc.ppc): a list of dicts in chain-block
        order.  Chains from n_valid on (padding) enter as the identity.  A draw that is not
        finite is an error."""
        parts, bad = self.ppc_partials_raw(row_begin, n_rows, n_valid)
        self.ppc_nonfinite = bad
        if bad:
            raise _lib.NestmcError("posterior predictive checks: %d draws were not finite" % bad)
        return parts

    def ppc(self, row_begin=0, n_rows=None, n_valid=None):
        """The PpcResult (nestmc.ppc) of this engine's chains: its chain blocks' partials
        merged in chain-block order."""
        from . import ppc as _ppc
        parts = self.ppc_partials(row_begin, n_rows, n_valid)
        return _ppc.finish(_ppc.merge(parts), self.off, self.observed())

    # -- held-out rows and new groups (nestmc.predict; csrc/predict.h) ----------------------
    def set_new_data(self, new_data):
        """The table to predict for (a nestmc.predict.NewData; None clears it): checked
        against the family and the pooling (ValueError), then copied to the device
        (nmc_predict_set)."""
        if new_data is None:
            check(self.lib.nmc_predict_set(self.h, None, 0, 0, None, 0))
            self.new_data = None
            return
        new_data.check(self.family, self.G, self.pooling)
        check(self.lib.nmc_predict_set(
            self.h, dptr(new_data.obs), new_data.n_new, new_data.n_fields,
            new_data.group.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), new_data.K))
        self.new_data = new_data

    def _new_data(self):
        nd = getattr(self, "new_data", None)
        if nd is None:
            raise ValueError("no new table: set_new_data(NewData(obs, group)) first")
        return nd

    def predict_draws(self, row_begin=0, n_rows=None, yrep=True, ll=True, theta_new=True):
        """At recorded rows of the sample store, for the new table (nmc_predict_draws): a dict
        of yrep [C, rows, n_new, NRESP] (the draws), ll [C, rows, n_new] (the log density of
        every new row) and theta_new [C, rows, K, P] (the new groups' values); an array not
        asked for is None.  For small windows, tests and statistics of one's own --
        Engine.predict never forms them.  yrep needs a family that can draw."""
        nd = self._new_data()
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        n_rows = max(int(n_rows), 0)
        NR = self.n_resp()
        y = numpy.empty((self.C, n_rows, nd.n_new, max(NR, 1))) if yrep else None
        L = numpy.empty((self.C, n_rows, nd.n_new)) if ll else None
        t = numpy.empty((self.C, n_rows, nd.K, self.P)) if theta_new else None
        check(self.lib.nmc_predict_draws(self.h, int(row_begin), n_rows, dptr(y), dptr(L),
                                         dptr(t)))
        return dict(yrep=y, ll=L, theta_new=t)

    def predict_partials_raw(self, row_begin=0, n_rows=None, n_valid=None):
        """nmc_predict_partials as it answers: (the chain blocks' partials, a list of
        nestmc.predict dicts in chain-block order, each with zero non-finite counts; the
        call's (non-finite draws, non-finite ll terms)).  A family that cannot draw gets the
        density alone (NRESP = 0 in the partials)."""
        nd = self._new_data()
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        if n_valid is None:
            n_valid = self.C
        CB, n, NR = (self.C + 63) // 64, nd.n_new, self.n_resp()
        dens = numpy.empty((CB, 2, n))
        st = numpy.empty((CB, 3, NR, n))
        ct = numpy.zeros((CB, 2, NR, n), dtype=numpy.uint32)
        bd, bl = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.nmc_predict_partials(
            self.h, int(row_begin), int(n_rows), int(n_valid), dptr(dens),
            dptr(st) if NR else None,
            ct.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if NR else None,
            ctypes.byref(bd), ctypes.byref(bl)))
        parts = []
        for b in range(CB):
            ns = float(int(n_rows) * min(64, max(0, int(n_valid) - 64 * b)))
            parts.append(dict(dens=numpy.concatenate([dens[b], numpy.full((1, n), ns)]),
                              state=st[b], count=ct[b].astype(numpy.int64),
                              nonfinite_draws=0, nonfinite_ll=0))
        return parts, (bd.value, bl.value)

    def predict_partials(self, row_begin=0, n_rows=None, n_valid=None):
        """The prediction partials of every chain block over recorded rows [row_begin,
        row_begin + n_rows) and local chains [0, n_valid), reduced on the device from the
        sample store (nmc_predict_partials; nestmc.predict): a list of dicts in chain-block
        order.  Chains from n_valid on (padding) enter as the identity.  A draw that is not
        finite, or a log density that is not finite at a row with a response, is an error."""
        parts, bad = self.predict_partials_raw(row_begin, n_rows, n_valid)
        self.predict_nonfinite = bad
        if bad[0] or bad[1]:
            raise _lib.NestmcError("prediction: %d draws and %d log densities were not finite"
                                   % bad)
        return parts

    def predict(self, row_begin=0, n_rows=None, n_valid=None):
        """The PredictionResult (nestmc.predict) of this engine's chains for the new table: its
        chain blocks' partials merged in chain-block order."""
        from . import predict as _predict
        parts = self.predict_partials(row_begin, n_rows, n_valid)
        return _predict.finish(_predict.merge(parts), self._new_data(),
                               self.family.response_fields())

    def loo_raw(self, row_begin=0, n_rows=None, n_valid=None, obs_batch=0):
        """PSIS-LOO's per-observation results over recorded rows [row_begin, row_begin +
        n_rows) and local chains [0, n_valid), computed on the device from the sample store
        (nmc_loo; nestmc.loo): a dict of elpd, lppd, k [n_obs], n_tail [n_obs] (int32) and
        nonfinite [n_obs] (an observation with NaN or infinite log-likelihoods has NaN
        results).  obs_batch: the observations sorted at a time (0: what fits the 1 GiB of
        temporary buffers); the results do not depend on it."""
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        if n_valid is None:
            n_valid = self.C
        n = int(self.off[-1])
        elpd, lppd, k = numpy.empty(n), numpy.empty(n), numpy.empty(n)
        nt = numpy.empty(n, dtype=numpy.int32)
        bad = numpy.empty(n, dtype=numpy.int64)
        check(self.lib.nmc_loo(self.h, int(row_begin), int(n_rows), int(n_valid), int(obs_batch),
                               dptr(elpd), dptr(lppd), dptr(k),
                               nt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                               bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return dict(elpd=elpd, lppd=lppd, k=k, n_tail=nt, nonfinite=bad,
                    n_samples=int(n_rows) * int(n_valid))

    def loo(self, row_begin=0, n_rows=None, n_valid=None, obs_batch=0):
        """The LooResult (nestmc.loo) of this engine's chains over the given rows.  A
        log-likelihood term that is not finite is an error."""
        from . import loo as _loo
        raw = self.loo_raw(row_begin, n_rows, n_valid, obs_batch)
        self.loo_nonfinite = int(raw["nonfinite"].sum())
        if self.loo_nonfinite:
            raise _lib.NestmcError("PSIS-LOO: %d per-observation log-likelihood terms were not "
                                   "finite" % self.loo_nonfinite)
        return _loo.LooResult(raw["elpd"], raw["lppd"], raw["k"], raw["n_tail"],
                              raw["n_samples"], self.off)

    def loo_pit_raw(self, row_begin=0, n_rows=None, n_valid=None, obs_batch=0):
        """nmc_loo_pit as it answers, over recorded rows [row_begin, row_begin + n_rows) and
        local chains [0, n_valid): loo_raw's dict (the same bits, from the same sort) with ess
        [n_obs] and wlt, weq, mean, var [n_obs, NRESP] and nonfinite_draws [n_obs, NRESP]
        (int64) of nestmc.loopit.  An observation with log-likelihoods that are not finite, or
        a field with replicates that are not finite, has NaN results.  obs_batch as in
        loo_raw; the results do not depend on it.  A family that cannot draw (a
        DeviceLikelihood without nmc_user_predict) raises ValueError."""
        if not self.family.response_fields():
            raise ValueError("LOO-PIT needs a family that can draw from its likelihood: this "
                             "DeviceLikelihood's source does not define nmc_user_predict")
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        if n_valid is None:
            n_valid = self.C
        n, NR = int(self.off[-1]), max(self.n_resp(), 1)
        elpd, lppd, k, ess = (numpy.empty(n) for _ in range(4))
        wlt, weq, mean, var = (numpy.empty((n, NR)) for _ in range(4))
        nt = numpy.empty(n, dtype=numpy.int32)
        bad = numpy.empty(n, dtype=numpy.int64)
        badd = numpy.empty((n, NR), dtype=numpy.int64)
        i64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731
        check(self.lib.nmc_loo_pit(self.h, int(row_begin), int(n_rows), int(n_valid),
                                   int(obs_batch), dptr(elpd), dptr(lppd), dptr(k),
                                   nt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), i64(bad),
                                   dptr(ess), dptr(wlt), dptr(weq), dptr(mean), dptr(var),
                                   i64(badd)))
        return dict(elpd=elpd, lppd=lppd, k=k, n_tail=nt, nonfinite=bad, ess=ess, wlt=wlt,
                    weq=weq, mean=mean, var=var, nonfinite_draws=badd,
                    n_samples=int(n_rows) * int(n_valid))

    def loo_pit(self, row_begin=0, n_rows=None, n_valid=None, obs_batch=0):
        """The LooPitResult (nestmc.loopit) of this engine's chains over the given rows; its
        .loo is the LooResult of the same pass.  A log-likelihood term or a replicate that is
        not finite is an error."""
        from . import loo as _loo
        from . import loopit as _loopit
        raw = self.loo_pit_raw(row_begin, n_rows, n_valid, obs_batch)
        self.loo_nonfinite = int(raw["nonfinite"].sum())
        if self.loo_nonfinite:
            raise _lib.NestmcError("LOO-PIT: %d per-observation log-likelihood terms were not "
                                   "finite" % self.loo_nonfinite)
        self.loo_pit_nonfinite = int(raw["nonfinite_draws"].sum())
        if self.loo_pit_nonfinite:
            raise _lib.NestmcError("LOO-PIT: %d draws were not finite" % self.loo_pit_nonfinite)
        res = _loo.LooResult(raw["elpd"], raw["lppd"], raw["k"], raw["n_tail"],
                             raw["n_samples"], self.off)
        return _loopit.LooPitResult(res, raw["ess"], raw["wlt"], raw["weq"], raw["mean"],
                                    raw["var"], self.observed(), raw["nonfinite_draws"])

    def conv_partials(self, row_begin=0, n_rows=None, n_valid=None):
        """The convergence diagnostic's partial sums over recorded rows [row_begin, row_begin +
        n_rows) (n_rows even, two halves of n = n_rows / 2 >= 2 rows) and local chains
        [0, n_valid), reduced on the device from the sample store (nmc_conv_partials;
        nestmc.convergence): (vg [CB, cols, n], mean [cols, 2, C], m2 [cols, 2, C]).  Chains
        from n_valid on (padding) add +0.0 to vg; their mean and m2 entries are +0.0."""
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        if n_valid is None:
            n_valid = self.C
        n_rows = int(n_rows)
        n = max(n_rows // 2, 0)
        vg = numpy.empty(((self.C + 63) // 64, self.cols, n))
        mean = numpy.empty((self.cols, 2, self.C))
        m2 = numpy.empty((self.cols, 2, self.C))
        check(self.lib.nmc_conv_partials(self.h, int(row_begin), n_rows, int(n_valid),
                                         dptr(mean), dptr(m2), dptr(vg)))
        return vg, mean, m2

    def convergence(self, names=None, row_begin=0, n_rows=None, n_valid=None):
        """The ConvergenceResult (nestmc.convergence: rhat, effective n, mean, sd per column)
        of this engine's chains over the given rows: its chain blocks' variogram sums merged
        in chain-block order.  names: the columns' names (default "col<k>")."""
        from . import convergence as _conv
        vg, mean, m2 = self.conv_partials(row_begin, n_rows, n_valid)
        nv = self.C if n_valid is None else int(n_valid)
        if names is None:
            names = ["col%d" % k for k in range(self.cols)]
        return _conv.finish(_conv.merge(list(vg)), mean[:, :, :nv], m2[:, :, :nv],
                            vg.shape[2], names)

    def summary_raw(self, row_begin=0, n_rows=None, n_valid=None, hdi_p=95, ranks=None,
                    col_batch=0, want_sorted=False):
        """The order statistics of every column over recorded rows [row_begin, row_begin +
        n_rows) and local chains [0, n_valid), N = n_rows * n_valid values each, sorted on the
        device from the sample store (nmc_summary; nestmc.summary): a dict of at_ranks
        [cols, len(ranks)] (the sorted column at ``ranks``; default
        nestmc.summary.stat_ranks(N): the median's two, the minimum's, the maximum's), hdi
        [cols, 2] and hdi_at [cols] (the hdi_p % interval and the rank of its lower end),
        nonfinite [cols] (a column with NaN or infinite values has NaN statistics and hdi_at
        -1), sorted ([cols, N], every column in key order, with want_sorted; else None), N and
        gap.  col_batch: the columns sorted at a time (0: what fits the 1 GiB of temporary
        buffers)."""
        from . import summary as _summary
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        if n_valid is None:
            n_valid = self.C
        n_rows, n_valid = int(n_rows), int(n_valid)
        N = n_rows * n_valid
        if N < 2:
            raise ValueError("a summary needs at least two values per column (got %d)" % N)
        gap = _summary.gap_of(N, hdi_p)
        rk = numpy.ascontiguousarray(_summary.stat_ranks(N) if ranks is None else ranks,
                                     dtype=numpy.int64).reshape(-1)
        i64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731
        at = numpy.empty((self.cols, len(rk)))
        hdi = numpy.empty((self.cols, 2))
        hdi_at = numpy.empty(self.cols, dtype=numpy.int64)
        bad = numpy.empty(self.cols, dtype=numpy.int64)
        srt = numpy.empty((self.cols, N)) if want_sorted else None
        check(self.lib.nmc_summary(self.h, int(row_begin), n_rows, n_valid, gap, i64(rk),
                                   len(rk), int(col_batch), dptr(at), dptr(hdi), i64(hdi_at),
                                   i64(bad), dptr(srt)))
        return dict(at_ranks=at, hdi=hdi, hdi_at=hdi_at, nonfinite=bad, sorted=srt, N=N, gap=gap)

    def summary(self, names=None, row_begin=0, n_rows=None, n_valid=None, hdi_p=95, col_batch=0):
        """The SummaryResult (nestmc.summary: median, HDI, minimum, maximum per column) of this
        engine's chains over the given rows.  names: the columns' names (default "col<k>")."""
        from . import summary as _summary
        raw = self.summary_raw(row_begin, n_rows, n_valid, hdi_p, None, col_batch)
        return _summary.finish(raw["at_ranks"], raw["hdi"], raw["nonfinite"], raw["N"], names,
                               hdi_p)

    def rank_partials(self, row_begin=0, n_rows=None, n_valid=None, col_batch=0):
        """The rank-normalised diagnostics' partial sums over recorded rows [row_begin,
        row_begin + n_rows) (n_rows even, two halves of n = n_rows / 2 >= 2 rows) and local
        chains [0, n_valid), on the device from the sample store (nmc_rank_partials;
        nestmc.rankdiag): (vg [4, CB, cols, n], mean [4, cols, 2, C], m2 [4, cols, 2, C],
        nonfinite [cols]), the first axis the derived quantities z, zf, I05, I95.  col_batch:
        the columns handled at a time (0: what fits the 1 GiB of temporary buffers); the
        results do not depend on it."""
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        if n_valid is None:
            n_valid = self.C
        n_rows = int(n_rows)
        n = max(n_rows // 2, 0)
        vg = numpy.empty((4, (self.C + 63) // 64, self.cols, n))
        mean = numpy.empty((4, self.cols, 2, self.C))
        m2 = numpy.empty((4, self.cols, 2, self.C))
        bad = numpy.empty(self.cols, dtype=numpy.int64)
        check(self.lib.nmc_rank_partials(self.h, int(row_begin), n_rows, int(n_valid),
                                         int(col_batch), dptr(vg), dptr(mean), dptr(m2),
                                         bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return vg, mean, m2, bad

    def rank_diagnostics(self, names=None, row_begin=0, n_rows=None, n_valid=None, col_batch=0):
        """The RankDiagnosticsResult (nestmc.rankdiag: rank-normalised and folded R-hat, bulk-
        and tail-ESS per column) of this engine's chains over the given rows.  names: the
        columns' names (default "col<k>")."""
        from . import rankdiag as _rankdiag
        vg, mean, m2, bad = self.rank_partials(row_begin, n_rows, n_valid, col_batch)
        nv = self.C if n_valid is None else int(n_valid)
        return _rankdiag.finish(vg, mean, m2, vg.shape[3], names, nv, bad)

    def group_order_counts(self, row_begin=0, n_rows=None, n_valid=None):
        """The groups' rank histogram and pairwise win counts over recorded rows [row_begin,
        row_begin + n_rows) and local chains [0, n_valid), counted on the device from the
        sample store (nmc_group_order; nestmc.groupcmp has the definitions): a dict of hist
        [P, G, G], wins [P, G, G], nonfinite [P] (int64) and n_samples."""
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        if n_valid is None:
            n_valid = self.C
        n_rows, n_valid = int(n_rows), int(n_valid)
        hist = numpy.empty((self.P, self.G, self.G), dtype=numpy.uint32)
        wins = numpy.empty((self.P, self.G, self.G), dtype=numpy.uint32)
        bad = numpy.empty(self.P, dtype=numpy.int64)
        u32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))   # noqa: E731
        check(self.lib.nmc_group_order(self.h, int(row_begin), n_rows, n_valid, u32(hist),
                                       u32(wins),
                                       bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return dict(hist=hist.astype(numpy.int64), wins=wins.astype(numpy.int64), nonfinite=bad,
                    n_samples=n_rows * n_valid)

    def group_comparison(self, names=None, row_begin=0, n_rows=None, n_valid=None):
        """The GroupComparisonResult (nestmc.groupcmp: every group's rank distribution and
        P(theta_g > theta_h) of every pair, per parameter) of this engine's chains over the
        given rows.  names: the P parameters' names (default "p<k>").  A group value that is
        not finite is an error."""
        from . import groupcmp as _groupcmp
        raw = self.group_order_counts(row_begin, n_rows, n_valid)
        self.group_nonfinite = int(raw["nonfinite"].sum())
        if self.group_nonfinite:
            raise _lib.NestmcError("group comparison: %d group values were not finite"
                                   % self.group_nonfinite)
        return _groupcmp.finish(raw["hist"], raw["wins"], raw["n_samples"], names)

    def comoments(self, row_begin=0, n_rows=None, n_valid=None):
        """The columns' moments and centred comoments over recorded rows [row_begin, row_begin
        + n_rows) and local chains [0, n_valid), on the device from the sample store
        (nmc_comoments; nestmc.correlation has the definitions): a dict of mean, min, max
        [cols], M [cols, cols], nonfinite [cols] (int64) and n_samples."""
        if n_rows is None:
            n_rows = self.n_rows - row_begin
        if n_valid is None:
            n_valid = self.C
        n_rows, n_valid = int(n_rows), int(n_valid)
        cols = self.cols
        mean = numpy.empty(cols)
        minmax = numpy.empty((2, cols))
        M = numpy.empty((cols, cols))
        bad = numpy.empty(cols, dtype=numpy.int64)
        check(self.lib.nmc_comoments(self.h, int(row_begin), n_rows, n_valid, _lib.dptr(mean),
                                     _lib.dptr(minmax), _lib.dptr(M),
                                     bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return dict(mean=mean, min=minmax[0].copy(), max=minmax[1].copy(), M=M, nonfinite=bad,
                    n_samples=n_rows * n_valid)

    def correlation(self, names=None, row_begin=0, n_rows=None, n_valid=None):
        """The CorrelationResult (nestmc.correlation: mean, sd, covariance and correlation
        matrix of all columns) of this engine's chains over the given rows.  names: the
        columns' names (default "c<k>").  A value that is not finite is an error."""
        from . import correlation as _correlation
        raw = self.comoments(row_begin, n_rows, n_valid)
        self.correlation_nonfinite = int(raw["nonfinite"].sum())
        if self.correlation_nonfinite:
            raise _lib.NestmcError("correlation: %d values were not finite"
                                   % self.correlation_nonfinite)
        return _correlation.finish(raw, names)

    def eval_obs_ll(self):
        """Per-observation LL at the current state: [C, n_obs]."""
        out = numpy.empty((self.C, int(self.off[-1])))
        check(self.lib.nmc_eval_obs_ll(self.h, dptr(out)))
        return out

    # -- timing ---------------------------------------------------------------
    def event_record(self, slot):
        check(self.lib.nmc_event_record(self.h, slot))

    def event_elapsed_ms(self, a, b):
        ms = ctypes.c_float()
        check(self.lib.nmc_event_elapsed(self.h, a, b, ctypes.byref(ms)))
        return ms.value

    def set_launch_iters(self, n):
        """Cap the iterations one persistent launch covers (0: the variate chunk)."""
        check(self.lib.nmc_set_launch_iters(self.h, int(n)))

    def set_kernel_timing(self, enable):
        check(self.lib.nmc_set_kernel_timing(self.h, 1 if enable else 0))

    def kernel_timing(self):
        sm, hm = ctypes.c_double(), ctypes.c_double()
        sn, si, hn = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.nmc_get_kernel_timing(self.h, ctypes.byref(sm), ctypes.byref(sn),
                                             ctypes.byref(si), ctypes.byref(hm),
                                             ctypes.byref(hn)))
        return dict(step_ms=sm.value, step_launches=sn.value, step_iters=si.value,
                    hyper_ms=hm.value, hyper_launches=hn.value)

    def gibbs_fallbacks(self):
        """(launch, chain block) pairs whose Gibbs tasks the step kernel updated itself
        because the separate Gibbs kernel did not run beside it (nmc_gibbs_fallbacks)."""
        n = ctypes.c_int64()
        check(self.lib.nmc_gibbs_fallbacks(self.h, ctypes.byref(n)))
        return n.value

    def gibbs_separate(self):
        """Whether nmc_k_sweep's Gibbs workgroups run as a kernel of their own, on a second
        stream (nmc_gibbs_kernel), and not in the step kernel's grid."""
        n = ctypes.c_int()
        check(self.lib.nmc_gibbs_kernel(self.h, ctypes.byref(n)))
        return bool(n.value)

    def launch_config(self):
        w, cb, pe, cl, md = (ctypes.c_int() for _ in range(5))
        check(self.lib.nmc_launch_config(self.h, ctypes.byref(w), ctypes.byref(cb),
                                         ctypes.byref(pe), ctypes.byref(cl), ctypes.byref(md)))
        sm, sb = ctypes.c_int(), ctypes.c_int()
        check(self.lib.nmc_split_config(self.h, ctypes.byref(sm), ctypes.byref(sb)))
        buf = ctypes.create_string_buffer(160)
        check(self.lib.nmc_kernel_name(self.h, buf, len(buf)))
        zin = ctypes.c_int()
        check(self.lib.nmc_variate_source(self.h, ctypes.byref(zin)))
        return dict(waves_per_group=w.value, chain_blocks=cb.value, persistent=bool(pe.value),
                    chains_per_block=cl.value, mode=MODE_NAMES.get(md.value, str(md.value)),
                    split_members=sm.value, chain_blocks_per_launch=sb.value,
                    kernel=buf.value.decode(), zin=zin.value)
