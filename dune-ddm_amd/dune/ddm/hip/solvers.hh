// Device-resident solvers behind Dune::InverseOperator -- the two plugin points of the reference:
//
// (1) the subdomain / coarse solver selected by string through the dune-istl solver factory
//     (dune/ddm/schwarz.hh:85-92, galerkin_preconditioner.hh:338-346); in-tree precedent for registering a new one:
//     DUNE_REGISTER_DIRECT_SOLVER("strumpack", Dune::StrumpackCreator()) (dune/ddm/strumpack.hh:95-122).
//     Dune::HipSubdomainSolver<M> wraps the library's local factor solvers (ILU(0) in natural order; sparse Cholesky / L U with
//     host factorisation and device triangular solves) for a flattened BCRSMatrix; registered under "hip_ilu0", "hip_cholesky",
//     "hip_lu" when the dune-istl factory macros are visible.
// (2) the outer Krylov solver (examples/poisson.cc:311-319 obtains it from the same factory): Dune::HipCGSolver /
//     Dune::HipRestartedGMResSolver / Dune::HipRestartedFlexibleGMResSolver / Dune::HipBiCGSTABSolver run the WHOLE loop on the device
//     (ddm_cg_solve / ddm_gmres_solve / ddm_fgmres_solve / ddm_bicgstab_solve: dune-istl's recurrences,
//     SURVEY.md 3.2) -- one upload of x and b, one download of x and the defect, instead of two PCIe copies of n_o doubles per
//     virtual apply() when dune-istl's own host solvers drive the adaptors.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include <dune/common/exceptions.hh>
#include <dune/common/parametertree.hh>
#include <dune/istl/operators.hh>
#include <dune/istl/preconditioner.hh>
#include <dune/istl/solver.hh>

#include "backend.hh"
#include "combined_preconditioner.hh"

namespace Dune {

template <class M, class X = BlockVector<FieldVector<double, 1>>>
class HipSubdomainSolver : public InverseOperator<X, X> {
public:
  // kind: "ilu0" | "cholesky" | "lu" | "direct" (Cholesky if the values are symmetric, else L U)
  explicit HipSubdomainSolver(const M& A, const std::string& kind = "ilu0") : ctx(ddm_hip::Context::get()), dA(ctx, A), n(A.N()), dd(ctx, A.N()), dx(ctx, A.N())
  {
    const int64_t bp[2] = {0, (int64_t)n};
    if (kind == "ilu0") ddm_hip::check(ctx->handle(), ddm_ilu0_create(ctx->handle(), dA.handle(), 1, bp, &F), "ddm_ilu0_create");
    else if (kind == "cholesky") ddm_hip::check(ctx->handle(), ddm_direct_create(ctx->handle(), dA.handle(), 1, bp, 0, 0.0, &F), "ddm_direct_create");
    else if (kind == "lu") ddm_hip::check(ctx->handle(), ddm_direct_create(ctx->handle(), dA.handle(), 1, bp, 1, 0.0, &F), "ddm_direct_create");
    else if (kind == "direct") {
      if (ddm_direct_create(ctx->handle(), dA.handle(), 1, bp, 0, 0.0, &F) != DDM_OK)
        ddm_hip::check(ctx->handle(), ddm_direct_create(ctx->handle(), dA.handle(), 1, bp, 1, 0.0, &F), "ddm_direct_create");
    } else DUNE_THROW(NotImplemented, "Unknown device subdomain solver '" + kind + "'");
  }
  ~HipSubdomainSolver() override { ddm_ilu0_destroy(F); }
  SolverCategory::Category category() const override { return SolverCategory::sequential; }
  void apply(X& x, X& b, InverseOperatorResult& res) override
  {
    dd.upload(b);
    ddm_hip::check(ctx->handle(), ddm_ilu0_solve(ctx->handle(), F, dd.data(), dx.data()), "ddm_ilu0_solve");
    dx.download(x);
    int st = 0;
    ddm_hip::check(ctx->handle(), ddm_ilu0_status(ctx->handle(), F, &st), "ddm_ilu0_status");
    res.iterations = 1;
    res.converged = st == 0;
  }
  void apply(X& x, X& b, [[maybe_unused]] double reduction, InverseOperatorResult& res) override { apply(x, b, res); }
  ddm_ilu0* handle() const { return F; }

private:
  std::shared_ptr<ddm_hip::Context> ctx;
  ddm_hip::DeviceCsr dA;
  std::size_t n;
  ddm_hip::DeviceVector dd, dx;
  ddm_ilu0* F = nullptr;
};

#ifdef DUNE_REGISTER_DIRECT_SOLVER
// factory registration, mirroring StrumpackCreator (dune/ddm/strumpack.hh:95-122)
template <int KIND>
struct HipSubdomainSolverCreator {
  template <typename TL, typename M>
  std::shared_ptr<Dune::InverseOperator<typename Dune::TypeListElement<1, TL>::type, typename Dune::TypeListElement<2, TL>::type>> operator()(
      TL /*tl*/, const M& mat, const Dune::ParameterTree& /*config*/, std::enable_if_t<std::is_same_v<typename M::field_type, double>, int> = 0) const
  {
    return std::make_shared<Dune::HipSubdomainSolver<M>>(mat, KIND == 0 ? "ilu0" : (KIND == 1 ? "cholesky" : "lu"));
  }
  template <typename TL, typename M>
  std::shared_ptr<Dune::InverseOperator<typename Dune::TypeListElement<1, TL>::type, typename Dune::TypeListElement<2, TL>::type>> operator()(
      TL /*tl*/, const M& /*mat*/, const Dune::ParameterTree& /*config*/, std::enable_if_t<!std::is_same_v<typename M::field_type, double>, int> = 0) const
  {
    DUNE_THROW(UnsupportedType, "Unsupported type in HipSubdomainSolver (double only)");
  }
};
DUNE_REGISTER_DIRECT_SOLVER("hip_ilu0", Dune::HipSubdomainSolverCreator<0>());
DUNE_REGISTER_DIRECT_SOLVER("hip_cholesky", Dune::HipSubdomainSolverCreator<1>());
DUNE_REGISTER_DIRECT_SOLVER("hip_lu", Dune::HipSubdomainSolverCreator<2>());
#endif

// Outer Krylov loops on the device.  op must be this directory's NonOverlappingOperator, prec its CombinedPreconditioner.
template <class X>
class HipKrylovSolverBase : public InverseOperator<X, X> {
public:
  HipKrylovSolverBase(std::shared_ptr<LinearOperator<X, X>> op_, std::shared_ptr<Preconditioner<X, X>> prec_, double reduction, int maxit, int verbose)
      : op(std::move(op_)), prec(std::move(prec_)), reduction_(reduction), maxit_(maxit), verbose_(verbose)
  {
    dop = dynamic_cast<ddm_hip::DeviceOperator*>(op.get());
    cprec = dynamic_cast<CombinedPreconditioner<X>*>(prec.get());
    if (!dop || !cprec) DUNE_THROW(NotImplemented, "the device Krylov solvers need the device NonOverlappingOperator and CombinedPreconditioner");
  }
  SolverCategory::Category category() const override { return op->category(); }
  void apply(X& x, X& b, InverseOperatorResult& res) override { apply(x, b, reduction_, res); }
  void apply(X& x, X& b, double reduction, InverseOperatorResult& res) override
  {
    auto ctx = cprec->context();
    const std::size_t n = b.N();
    if (!dx || dx->size() != n) {
      dx = std::make_unique<ddm_hip::DeviceVector>(ctx, n);
      db = std::make_unique<ddm_hip::DeviceVector>(ctx, n);
    }
    prec->pre(x, b);
    dx->upload(x);   // the only host -> device copies of the solve
    db->upload(b);
    ddm_solve_result r{};
    ddm_hip::check(ctx->handle(), solve(ctx->handle(), dop->op_handle(), cprec->handle(n), dx->data(), db->data(), reduction, &r), "device Krylov solve");
    dx->download(x);   // the only device -> host copies
    db->download(b);   // dune-istl leaves the defect in b
    prec->post(x);
    res.clear();
    res.iterations = r.iterations;
    res.converged = r.converged != 0;
    res.reduction = r.reduction;
    res.elapsed = r.elapsed_s;
    res.conv_rate = r.iterations > 0 ? std::pow(r.reduction, 1.0 / r.iterations) : 0.0;
    if (verbose_ > 0) std::printf("=== device Krylov solve: %d iterations, reduction %.3e, %.3f s\n", r.iterations, r.reduction, r.elapsed_s);
  }

  // Several right-hand sides at once: x.size() independent solves (1 to 32 columns) in one device loop (HipCGSolver: ddm_cg_solve_multi;
  // HipRestartedGMResSolver: ddm_gmres_solve_multi; HipRestartedFlexibleGMResSolver: ddm_fgmres_solve_multi; HipRestartedFCGSolver / HipCompleteFCGSolver: ddm_fcg_solve_multi), each column as apply(x[c], b[c], reduction, res[c]) would run it.  One upload and
  // one download of the whole row-major n x m block; b receives what the solver left there (the defects).  HipBlockCGSolver is the one
  // solver whose columns are NOT independent: ddm_bcg_solve_multi, one shared search space; HipBlockGMResSolver likewise (ddm_bgmres_solve_multi).  A solver without a block
  // loop (HipBiCGSTABSolver) throws Dune::NotImplemented.
  void apply(std::vector<X>& x, std::vector<X>& b, double reduction, std::vector<InverseOperatorResult>& res)
  {
    const std::size_t m = b.size();
    if (m < 1 || m > 32 || x.size() != m) DUNE_THROW(InvalidStateException, "device Krylov block apply: 1 to 32 columns, as many x as b");
    const std::size_t n = b[0].N();
    for (std::size_t c = 0; c < m; ++c)
      if (b[c].N() != n || x[c].N() != n) DUNE_THROW(InvalidStateException, "device Krylov block apply: the columns differ in size");
    auto ctx = cprec->context();
    ddm_hip::DeviceVector dX(ctx, n * m), dB(ctx, n * m);
    std::vector<double> hx(n * m), hb(n * m);
    for (std::size_t c = 0; c < m; ++c) {
      prec->pre(x[c], b[c]);
      for (std::size_t i = 0; i < n; ++i) {
        hx[i * m + c] = x[c][i][0];
        hb[i * m + c] = b[c][i][0];
      }
    }
    ddm_hip::check(ctx->handle(), ddm_memcpy_h2d(ctx->handle(), dX.data(), hx.data(), (int64_t)(n * m * sizeof(double))), "h2d");
    ddm_hip::check(ctx->handle(), ddm_memcpy_h2d(ctx->handle(), dB.data(), hb.data(), (int64_t)(n * m * sizeof(double))), "h2d");
    std::vector<ddm_solve_result> r(m);
    ddm_hip::check(ctx->handle(), solve_block(ctx->handle(), dop->op_handle(), cprec->handle(n), (int)m, dX.data(), dB.data(), reduction, r.data()), "device block Krylov solve");
    ddm_hip::check(ctx->handle(), ddm_memcpy_d2h(ctx->handle(), hx.data(), dX.data(), (int64_t)(n * m * sizeof(double))), "d2h");
    ddm_hip::check(ctx->handle(), ddm_memcpy_d2h(ctx->handle(), hb.data(), dB.data(), (int64_t)(n * m * sizeof(double))), "d2h");
    res.assign(m, InverseOperatorResult{});
    for (std::size_t c = 0; c < m; ++c) {
      for (std::size_t i = 0; i < n; ++i) {
        x[c][i][0] = hx[i * m + c];
        b[c][i][0] = hb[i * m + c];
      }
      prec->post(x[c]);
      res[c].clear();
      res[c].iterations = r[c].iterations;
      res[c].converged = r[c].converged != 0;
      res[c].reduction = r[c].reduction;
      res[c].elapsed = r[c].elapsed_s;
      res[c].conv_rate = r[c].iterations > 0 ? std::pow(r[c].reduction, 1.0 / r[c].iterations) : 0.0;
    }
    if (verbose_ > 0) std::printf("=== device block Krylov solve: %zu columns, %.3f s\n", m, m ? r[0].elapsed_s : 0.0);
  }

  // Any number of right-hand sides through a block loop of `width` (1 to 32) slots (HipCGSolver: ddm_cg_solve_queue; HipBiCGSTABSolver:
  // ddm_bicgstab_solve_queue): a slot whose column has stopped takes the next pending one.  Each column as apply(x[c], b[c], res[c])
  // with the solver's reduction would run it, except that b is left as it is (the defects live in the device work block).  One upload
  // of both row-major n x M blocks, one download of x.  A solver without a queued loop (the GMRES solvers: their restart cycles are
  // aligned) throws Dune::NotImplemented.
  void apply_queue(std::vector<X>& x, std::vector<X>& b, int width, std::vector<InverseOperatorResult>& res)
  {
    const std::size_t m = b.size();
    if (m < 1 || x.size() != m || width < 1 || width > 32)
      DUNE_THROW(InvalidStateException, "device Krylov queued apply: at least one column, as many x as b, a width of 1 to 32");
    const std::size_t n = b[0].N();
    for (std::size_t c = 0; c < m; ++c)
      if (b[c].N() != n || x[c].N() != n) DUNE_THROW(InvalidStateException, "device Krylov queued apply: the columns differ in size");
    auto ctx = cprec->context();
    ddm_hip::DeviceVector dX(ctx, n * m), dB(ctx, n * m);
    std::vector<double> hx(n * m), hb(n * m);
    for (std::size_t c = 0; c < m; ++c) {
      prec->pre(x[c], b[c]);
      for (std::size_t i = 0; i < n; ++i) {
        hx[i * m + c] = x[c][i][0];
        hb[i * m + c] = b[c][i][0];
      }
    }
    ddm_hip::check(ctx->handle(), ddm_memcpy_h2d(ctx->handle(), dX.data(), hx.data(), (int64_t)(n * m * sizeof(double))), "h2d");
    ddm_hip::check(ctx->handle(), ddm_memcpy_h2d(ctx->handle(), dB.data(), hb.data(), (int64_t)(n * m * sizeof(double))), "h2d");
    std::vector<ddm_solve_result> r(m);
    ddm_hip::check(ctx->handle(),
                   solve_queue(ctx->handle(), dop->op_handle(), cprec->handle(n), (int64_t)m, width, dX.data(), dB.data(), reduction_, r.data()),
                   "device queued Krylov solve");
    ddm_hip::check(ctx->handle(), ddm_memcpy_d2h(ctx->handle(), hx.data(), dX.data(), (int64_t)(n * m * sizeof(double))), "d2h");
    res.assign(m, InverseOperatorResult{});
    for (std::size_t c = 0; c < m; ++c) {
      for (std::size_t i = 0; i < n; ++i) x[c][i][0] = hx[i * m + c];
      prec->post(x[c]);
      res[c].clear();
      res[c].iterations = r[c].iterations;
      res[c].converged = r[c].converged != 0;
      res[c].reduction = r[c].reduction;
      res[c].elapsed = r[c].elapsed_s;
      res[c].conv_rate = r[c].iterations > 0 ? std::pow(r[c].reduction, 1.0 / r[c].iterations) : 0.0;
    }
    if (verbose_ > 0) std::printf("=== device queued Krylov solve: %zu columns through %d slots, %.3f s\n", m, width, r[0].elapsed_s);
  }

protected:
  virtual int solve(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, double* x, double* b, double reduction, ddm_solve_result* r) = 0;
  // the block loop of the solver on row-major n x m device blocks (r: m entries)
  virtual int solve_block(ddm_ctx*, ddm_op*, ddm_combined*, int, double*, double*, double, ddm_solve_result*)
  {
    DUNE_THROW(NotImplemented, "this device Krylov solver has no loop for several right-hand sides (cgsolver, restartedgmressolver, restartedflexiblegmressolver, restartedfcgsolver and completefcgsolver have one)");
  }
  // the queued loop of the solver: row-major n x ncols device blocks through `width` slots (r: ncols entries)
  virtual int solve_queue(ddm_ctx*, ddm_op*, ddm_combined*, int64_t, int, double*, double*, double, ddm_solve_result*)
  {
    DUNE_THROW(NotImplemented, "this device Krylov solver has no queued loop for any number of right-hand sides (cgsolver and bicgstabsolver have one)");
  }
  std::shared_ptr<LinearOperator<X, X>> op;
  std::shared_ptr<Preconditioner<X, X>> prec;
  ddm_hip::DeviceOperator* dop = nullptr;
  CombinedPreconditioner<X>* cprec = nullptr;
  double reduction_;
  int maxit_, verbose_;
  std::unique_ptr<ddm_hip::DeviceVector> dx, db;
};

// [solver] type = cgsolver (examples/poisson.ini:12-17): dune-istl CGSolver::apply
template <class X>
class HipCGSolver : public HipKrylovSolverBase<X> {
public:
  HipCGSolver(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, double reduction, int maxit, int verbose = 0)
      : HipKrylovSolverBase<X>(std::move(op), std::move(prec), reduction, maxit, verbose) {}
  HipCGSolver(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, const ParameterTree& cfg)
      : HipCGSolver(std::move(op), std::move(prec), cfg.get("reduction", 1e-8), cfg.get("maxit", 1000), cfg.get("verbose", 0)) {}

  using HipKrylovSolverBase<X>::apply;

protected:
  int solve(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, double* x, double* b, double reduction, ddm_solve_result* r) override
  {
    return ddm_cg_solve(ctx, o, p, x, b, reduction, this->maxit_, 0, nullptr, r);
  }
  int solve_block(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, int m, double* X_, double* B_, double reduction, ddm_solve_result* r) override
  {
    return ddm_cg_solve_multi(ctx, o, p, m, X_, B_, reduction, this->maxit_, nullptr, r);
  }
  int solve_queue(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, int64_t ncols, int width, double* X_, double* B_, double reduction, ddm_solve_result* r) override
  {
    return ddm_cg_solve_queue(ctx, o, p, ncols, width, X_, B_, reduction, this->maxit_, nullptr, r);
  }
};

// Restarted GMRES, left-preconditioned or flexible: the two solvers below are this class with the two C functions they call
template <class X, decltype(&ddm_gmres_solve) SOLVE, decltype(&ddm_gmres_solve_multi) SOLVE_BLOCK>
class HipRestartedGMResSolverBase : public HipKrylovSolverBase<X> {
public:
  HipRestartedGMResSolverBase(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, double reduction, int restart, int maxit, int verbose = 0)
      : HipKrylovSolverBase<X>(std::move(op), std::move(prec), reduction, maxit, verbose), restart_(restart) {}
  HipRestartedGMResSolverBase(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, const ParameterTree& cfg)
      : HipRestartedGMResSolverBase(std::move(op), std::move(prec), cfg.get("reduction", 1e-8), cfg.get("restart", 30), cfg.get("maxit", 1000), cfg.get("verbose", 0)) {}

protected:
  int solve(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, double* x, double* b, double reduction, ddm_solve_result* r) override
  {
    return SOLVE(ctx, o, p, x, b, reduction, this->maxit_, restart_, nullptr, r);
  }
  int solve_block(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, int m, double* X_, double* B_, double reduction, ddm_solve_result* r) override
  {
    return SOLVE_BLOCK(ctx, o, p, m, X_, B_, reduction, this->maxit_, restart_, nullptr, r);
  }
  int restart_;
};

// [solver] type = restartedgmressolver (default of TwoLevelSchwarzSolver, dune/ddm/twolevel_schwarz.hh:121-130)
template <class X>
class HipRestartedGMResSolver : public HipRestartedGMResSolverBase<X, &ddm_gmres_solve, &ddm_gmres_solve_multi> {
public:
  using HipRestartedGMResSolverBase<X, &ddm_gmres_solve, &ddm_gmres_solve_multi>::HipRestartedGMResSolverBase; // both constructors
  using HipKrylovSolverBase<X>::apply;
};

// [solver] type = restartedflexiblegmressolver: dune-istl RestartedFlexibleGMResSolver::apply -- right-preconditioned, the TRUE defect is
// monitored (as in HipCGSolver), and the preconditioner may change between iterations (ddm_schwarz_set_multi_precision); twice the
// basis memory of HipRestartedGMResSolver
template <class X>
class HipRestartedFlexibleGMResSolver : public HipRestartedGMResSolverBase<X, &ddm_fgmres_solve, &ddm_fgmres_solve_multi> {
public:
  using HipRestartedGMResSolverBase<X, &ddm_fgmres_solve, &ddm_fgmres_solve_multi>::HipRestartedGMResSolverBase; // both constructors
  using HipKrylovSolverBase<X>::apply;
};

// Flexible CG, restarted or complete: the two solvers below are this class with the variant flag of ddm_fcg_solve / ddm_fcg_solve_multi.
// For a symmetric positive definite operator with a preconditioner that is not symmetric (restricted Schwarz, the multiplicative
// combination) or not fixed (ddm_schwarz_set_multi_precision); the TRUE defect is tested; 2 (mmax + 1) vectors per column.
template <class X, int COMPLETE>
class HipFCGSolverBase : public HipKrylovSolverBase<X> {
public:
  HipFCGSolverBase(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, double reduction, int maxit, int verbose = 0, int mmax = 10)
      : HipKrylovSolverBase<X>(std::move(op), std::move(prec), reduction, maxit, verbose), mmax_(mmax) {}
  HipFCGSolverBase(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, const ParameterTree& cfg)
      : HipFCGSolverBase(std::move(op), std::move(prec), cfg.get("reduction", 1e-8), cfg.get("maxit", 1000), cfg.get("verbose", 0), cfg.get("mmax", 10)) {}

protected:
  int solve(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, double* x, double* b, double reduction, ddm_solve_result* r) override
  {
    return ddm_fcg_solve(ctx, o, p, x, b, reduction, this->maxit_, mmax_, COMPLETE, nullptr, r);
  }
  int solve_block(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, int m, double* X_, double* B_, double reduction, ddm_solve_result* r) override
  {
    return ddm_fcg_solve_multi(ctx, o, p, m, X_, B_, reduction, this->maxit_, mmax_, COMPLETE, nullptr, r);
  }
  int mmax_;
};

// [solver] type = restartedfcgsolver: dune-istl RestartedFCGSolver::apply (mmax: the slots kept, default 10)
template <class X>
class HipRestartedFCGSolver : public HipFCGSolverBase<X, 0> {
public:
  using HipFCGSolverBase<X, 0>::HipFCGSolverBase; // both constructors
  using HipKrylovSolverBase<X>::apply;            // (apply_queue throws Dune::NotImplemented: there is no queued flexible CG loop)
};

// [solver] type = completefcgsolver: dune-istl CompleteFCGSolver::apply -- the window keeps the stale higher slots after a wrap
template <class X>
class HipCompleteFCGSolver : public HipFCGSolverBase<X, 1> {
public:
  using HipFCGSolverBase<X, 1>::HipFCGSolverBase; // both constructors
  using HipKrylovSolverBase<X>::apply;
};

// [solver] type = blockcgsolver: block CG (ddm_bcg_solve_multi), a true block-Krylov method -- the columns of the block apply share ONE
// search space, so the iteration count falls as columns are added; not a dune-istl solver.  For a symmetric positive definite
// preconditioner, as HipCGSolver.  rank_tol: relative eigenvalue of the scaled coupling matrix below which a direction counts as
// dependent.  res[c].iterations is the first iteration at which column c passed its test.  The single-vector apply is the block of
// width 1 (CG); apply_queue throws Dune::NotImplemented (there is no queued block CG).
template <class X>
class HipBlockCGSolver : public HipKrylovSolverBase<X> {
public:
  HipBlockCGSolver(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, double reduction, int maxit, int verbose = 0,
                   double rank_tol = DDM_BCG_RANK_TOL_DEFAULT)
      : HipKrylovSolverBase<X>(std::move(op), std::move(prec), reduction, maxit, verbose), rank_tol_(rank_tol) {}
  HipBlockCGSolver(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, const ParameterTree& cfg)
      : HipBlockCGSolver(std::move(op), std::move(prec), cfg.get("reduction", 1e-8), cfg.get("maxit", 1000), cfg.get("verbose", 0),
                         cfg.get("rank_tol", DDM_BCG_RANK_TOL_DEFAULT)) {}

  using HipKrylovSolverBase<X>::apply;

protected:
  int solve(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, double* x, double* b, double reduction, ddm_solve_result* r) override
  {
    return ddm_bcg_solve_multi(ctx, o, p, 1, x, b, reduction, this->maxit_, rank_tol_, nullptr, nullptr, r);
  }
  int solve_block(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, int m, double* X_, double* B_, double reduction, ddm_solve_result* r) override
  {
    return ddm_bcg_solve_multi(ctx, o, p, m, X_, B_, reduction, this->maxit_, rank_tol_, nullptr, nullptr, r);
  }
  double rank_tol_;
};

// [solver] type = blockgmressolver: block GMRES (ddm_bgmres_solve_multi), the companion of HipBlockCGSolver for a preconditioner or an
// operator that is not symmetric -- the columns of the block apply share ONE Krylov space; not a dune-istl solver.  Right preconditioning
// with a fixed preconditioner, the true defect is monitored.  restart: block iterations per cycle (default 30, as HipRestartedGMResSolver); maxit counts block iterations;
// rank_tol: relative eigenvalue of the scaled Gram matrix of a block below which a direction counts as dependent.  res[c].iterations
// is the first block iteration at which column c passed its test and stayed passed.  The single-vector apply is the block of width 1
// (right-preconditioned restarted GMRES); apply_queue throws Dune::NotImplemented (there is no queued block GMRES).
template <class X>
class HipBlockGMResSolver : public HipKrylovSolverBase<X> {
public:
  HipBlockGMResSolver(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, double reduction, int restart, int maxit,
                      int verbose = 0, double rank_tol = DDM_BGMRES_RANK_TOL_DEFAULT)
      : HipKrylovSolverBase<X>(std::move(op), std::move(prec), reduction, maxit, verbose), restart_(restart), rank_tol_(rank_tol) {}
  HipBlockGMResSolver(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, const ParameterTree& cfg)
      : HipBlockGMResSolver(std::move(op), std::move(prec), cfg.get("reduction", 1e-8), cfg.get("restart", 30), cfg.get("maxit", 1000),
                            cfg.get("verbose", 0), cfg.get("rank_tol", DDM_BGMRES_RANK_TOL_DEFAULT)) {}

  using HipKrylovSolverBase<X>::apply;

protected:
  int solve(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, double* x, double* b, double reduction, ddm_solve_result* r) override
  {
    return ddm_bgmres_solve_multi(ctx, o, p, 1, x, b, reduction, this->maxit_, restart_, rank_tol_, nullptr, nullptr, r);
  }
  int solve_block(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, int m, double* X_, double* B_, double reduction, ddm_solve_result* r) override
  {
    return ddm_bgmres_solve_multi(ctx, o, p, m, X_, B_, reduction, this->maxit_, restart_, rank_tol_, nullptr, nullptr, r);
  }
  int restart_;
  double rank_tol_;
};

// [solver] type = bicgstabsolver: dune-istl BiCGSTABSolver::apply
template <class X>
class HipBiCGSTABSolver : public HipKrylovSolverBase<X> {
public:
  HipBiCGSTABSolver(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, double reduction, int maxit, int verbose = 0)
      : HipKrylovSolverBase<X>(std::move(op), std::move(prec), reduction, maxit, verbose) {}
  HipBiCGSTABSolver(std::shared_ptr<LinearOperator<X, X>> op, std::shared_ptr<Preconditioner<X, X>> prec, const ParameterTree& cfg)
      : HipBiCGSTABSolver(std::move(op), std::move(prec), cfg.get("reduction", 1e-8), cfg.get("maxit", 1000), cfg.get("verbose", 0)) {}

  using HipKrylovSolverBase<X>::apply; // (the block overload throws Dune::NotImplemented: the block BiCGSTAB loop is apply_queue, any M through w slots)

protected:
  int solve(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, double* x, double* b, double reduction, ddm_solve_result* r) override
  {
    return ddm_bicgstab_solve(ctx, o, p, x, b, reduction, this->maxit_, nullptr, nullptr, r);
  }
  int solve_queue(ddm_ctx* ctx, ddm_op* o, ddm_combined* p, int64_t ncols, int width, double* X_, double* B_, double reduction, ddm_solve_result* r) override
  {
    return ddm_bicgstab_solve_queue(ctx, o, p, ncols, width, X_, B_, reduction, this->maxit_, nullptr, nullptr, r);
  }
};

// getSolverFromFactory(op, solver_subtree, prec) for the device solvers (examples/poisson.cc:311-316)
template <class X>
std::shared_ptr<InverseOperator<X, X>> getHipSolver(std::shared_ptr<LinearOperator<X, X>> op, const ParameterTree& cfg, std::shared_ptr<Preconditioner<X, X>> prec)
{
  const auto type = cfg.get("type", std::string("cgsolver"));
  if (type == "cgsolver") return std::make_shared<HipCGSolver<X>>(std::move(op), std::move(prec), cfg);
  if (type == "restartedgmressolver") return std::make_shared<HipRestartedGMResSolver<X>>(std::move(op), std::move(prec), cfg);
  if (type == "restartedflexiblegmressolver") return std::make_shared<HipRestartedFlexibleGMResSolver<X>>(std::move(op), std::move(prec), cfg);
  if (type == "restartedfcgsolver") return std::make_shared<HipRestartedFCGSolver<X>>(std::move(op), std::move(prec), cfg);
  if (type == "completefcgsolver") return std::make_shared<HipCompleteFCGSolver<X>>(std::move(op), std::move(prec), cfg);
  if (type == "bicgstabsolver") return std::make_shared<HipBiCGSTABSolver<X>>(std::move(op), std::move(prec), cfg);
  if (type == "blockcgsolver") return std::make_shared<HipBlockCGSolver<X>>(std::move(op), std::move(prec), cfg);
  if (type == "blockgmressolver") return std::make_shared<HipBlockGMResSolver<X>>(std::move(op), std::move(prec), cfg);
  DUNE_THROW(NotImplemented, "solver type '" + type + "' has no device implementation (cgsolver, restartedgmressolver, restartedflexiblegmressolver, restartedfcgsolver, completefcgsolver, bicgstabsolver, blockcgsolver, blockgmressolver)");
}

}  // namespace Dune
