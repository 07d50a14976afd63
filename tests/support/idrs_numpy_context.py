"""The NumPy test double with the IDR(s) entries added - TEST INFRASTRUCTURE ONLY (tests/test_idrs_host.py).
``idrs_init`` / ``_dir`` / ``_orth`` / ``_omega`` / ``_run`` follow the signatures of ``krypy_amd/_hip.py``'s ``Context`` with
the positions of tests/support/idrs_ref.py (``Stepper``) in place of the kernels and ``numpy.dot`` for the sums; the checks
are the library's, with its messages."""
from krypy_amd._hip import IDRS_NSCAL, IDRS_RUN_MAX, IDRS_SMAX, BackendError
from tests.support import idrs_ref as ref
from tests.support.bicgstab_numpy_context import BicgstabNumpyContext
from tests.support.numpy_context import _same


class IdrsNumpyContext(BicgstabNumpyContext):
    def _idrs_stepper(self, what, state):
        P, pcol, G, gcol, U, ucol, R, rcol, YK, ycol, T, tcol, SC, s = state
        if _same(what, P, G, U, R, YK, T, SC):
            raise BackendError("%s: real blocks expected" % what)
        who = "kh_" + what
        if not 1 <= s <= IDRS_SMAX:
            raise BackendError("%s: s = %d is outside 1 .. %d" % (who, s, IDRS_SMAX))
        blocks = [("P", P, pcol, s), ("G", G, gcol, s), ("U", U, ucol, s), ("r", R, rcol, 1), ("yk", YK, ycol, 1),
                  ("t", T, tcol, 1)]
        for name, B, c, cnt in blocks:
            if c < 0 or c + cnt > B.ncols:
                raise BackendError("%s(%s): columns [%d, %d) out of range (ncols=%d)" % (who, name, c, c + cnt, B.ncols))
        for name, B, c, cnt in blocks:
            if B.n != R.n:
                raise BackendError("%s: length mismatch (%s)" % (who, name))
        for i, (ni, Bi, ci, ki) in enumerate(blocks):
            for nj, Bj, cj, kj in blocks[i + 1:]:
                if Bi is Bj and not (ci + ki <= cj or cj + kj <= ci):
                    raise BackendError("%s: %s and %s share a column" % (who, ni, nj))
        if SC.n < IDRS_NSCAL:
            raise BackendError("%s: the scalar block is short (%d doubles, %d needed)" % (who, SC.n, IDRS_NSCAL))
        for name, B, _, _ in blocks:
            if B is SC:
                raise BackendError("%s: %s and the scalar block share a column" % (who, name))
        return ref.Stepper(P.a[:, pcol: pcol + s], G.a[:, gcol: gcol + s], U.a[:, ucol: ucol + s], R.a[:, rcol], YK.a[:, ycol],
                           T.a[:, tcol], SC.a[:, 0], self._dot)

    @staticmethod
    def _position(who, k, s):
        if not 0 <= k < s:
            raise BackendError("%s: position k = %d is outside 0 .. s - 1 = %d" % (who, k, s - 1))

    @staticmethod
    def _record(st):
        rec = st.sc[ref.L["REC"]: ref.L["REC"] + 4]
        return float(rec[0]), float(rec[1]), float(rec[2]), int(rec[3])

    def idrs_init(self, state):
        self._count("idrs_init")
        return self._idrs_stepper("idrs_init", state).init()

    def idrs_dir(self, state, k):
        self._count("idrs_dir")
        st = self._idrs_stepper("idrs_dir", state)
        self._position("kh_idrs_dir", k, st.s)
        st.clear_stop()
        st.dir(k)

    def idrs_orth(self, state, k, bnorm, tol):
        self._count("idrs_orth")
        st = self._idrs_stepper("idrs_orth", state)
        self._position("kh_idrs_orth", k, st.s)
        st.orth(k, float(bnorm), float(tol))
        return self._record(st)

    def idrs_omega(self, state, bnorm, tol):
        self._count("idrs_omega")
        st = self._idrs_stepper("idrs_omega", state)
        st.clear_stop()
        st.omega(float(bnorm), float(tol))
        return self._record(st)

    def idrs_run(self, A, state, pos, nsteps, bnorm, tol):
        self._count("idrs_run")
        st = self._idrs_stepper("idrs_run", state)
        if A.dtype.kind == "c":
            raise BackendError("kh_idrs_run: real operator expected")
        if A.shape != (st.r.size, st.r.size):
            raise BackendError("kh_idrs_run: length mismatch (operator)")
        if not 0 <= pos <= st.s:
            raise BackendError("kh_idrs_run: position %d is outside 0 .. s = %d" % (pos, st.s))
        if not 1 <= nsteps <= IDRS_RUN_MAX:
            raise BackendError("kh_idrs_run: nsteps = %d is outside 1 .. %d" % (nsteps, IDRS_RUN_MAX))
        st.clear_stop()
        for i in range(nsteps):
            st.position((pos + i) % (st.s + 1), lambda x: self._matvec(A, x), float(bnorm), float(tol))
        done = int(st.sc[ref.L["COUNT"]])
        self.__dict__.setdefault("_kv", {})["n_idrs_steps"] = self.get("n_idrs_steps") + done
        rec = st.sc[ref.L["REC"]: ref.L["REC"] + 4 * done].reshape(done, 4)
        return [(float(r[0]), float(r[1]), float(r[2]), int(r[3])) for r in rec]
