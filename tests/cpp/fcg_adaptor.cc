// Drives Dune::HipRestartedFCGSolver and Dune::HipCompleteFCGSolver ([solver] type = restartedfcgsolver / completefcgsolver) the way
// examples/poisson.cc:229-321 builds its solver: restricted SchwarzPreconditioner (ILU(0)) + POU GalerkinPreconditioner in a
// multiplicative CombinedPreconditioner -- a preconditioner that is not symmetric --, NonOverlappingOperator, the solver from
// getHipSolver with mmax = 3 so that the slots wrap.  Single rank (mock communication, see mock/).  The factory must return the two
// classes for the two keys; the single-vector and the block apply are checked BITWISE against ddm_fcg_solve / ddm_fcg_solve_multi
// called on the same device objects, and their iteration counts against the ones on the command line; apply_queue must throw
// Dune::NotImplemented.
//   usage: fcg_adaptor <dir with rowptr.bin col.bin val.bin b.bin dirichlet.bin pou.bin> <m> <1 + m counts restarted> <1 + m counts complete>
//          (per variant: the iterations of the single-vector solve of column 0, then of the m columns of the block solve)
// prints per variant "factory <key> <0|1>", "single <key> <iterations adaptor> <iterations C ABI> <expected> <entries of x that differ>
// <entries of b that differ>", per column "col <key> <c> <iterations adaptor> <iterations C ABI> <expected> <x differ> <b differ>" and
// "queue <key> <0|1>" (1: apply_queue threw Dune::NotImplemented), then "fcg_ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "adaptor_fixture.hh"   // first: the adaptor headers below expect the dune-istl ones before them

#include <dune/ddm/hip/solvers.hh>

static std::size_t differing(const double* a, const double* b, std::size_t n)
{
  std::size_t d = 0;
  for (std::size_t i = 0; i < n; ++i) d += std::memcmp(a + i, b + i, sizeof(double)) != 0;
  return d;
}

template <class Solver>
static bool variant(const char* key, int complete, const Problem& p, const std::vector<double>& bb, int m, const int* expected)
{
  const std::size_t n = p.n;
  auto ptree = two_level_ptree("restricted", "ilu0", "multiplicative", "umfpack");
  ptree.sub("solver")["type"] = key;
  ptree.sub("solver")["mmax"] = "3";
  ptree.sub("solver")["maxit"] = "500";
  ptree.sub("solver")["reduction"] = "1e-10";
  const TwoLevel t = build_two_level(p, ptree);
  std::shared_ptr<Dune::InverseOperator<Vec, Vec>> made =
      Dune::getHipSolver<Vec>(std::static_pointer_cast<Dune::LinearOperator<Vec, Vec>>(t.op), ptree.sub("solver"), std::static_pointer_cast<Dune::Preconditioner<Vec, Vec>>(t.prec));
  auto solver = std::dynamic_pointer_cast<Solver>(made);
  std::printf("factory %s %d\n", key, solver ? 1 : 0);
  if (!solver) return false;

  std::vector<Vec> B = seeded_columns(p, bb, m), X = zero_columns(n, m);
  std::vector<double> hb = pack(B), hx(n * m, 0.0);
  const std::vector<Vec> Bsave = B;
  auto ctx = t.prec->context();   // the same device objects through the C ABI
  ddm_ctx* h = ctx->handle();
  ddm_op* oh = t.op->op_handle();
  ddm_combined* ph = t.prec->handle(n);
  bool ok = true;
  {
    Vec x1(n), b1 = Bsave[0];
    x1 = 0;
    Dune::InverseOperatorResult r1;
    solver->apply(x1, b1, 1e-10, r1);
    ddm_hip::DeviceVector dx(ctx, n), db(ctx, n);
    std::vector<double> cx(n, 0.0), cb(n);
    for (std::size_t i = 0; i < n; ++i) cb[i] = Bsave[0][i];
    ddm_hip::check(h, ddm_memcpy_h2d(h, dx.data(), cx.data(), (int64_t)(n * sizeof(double))), "h2d");
    ddm_hip::check(h, ddm_memcpy_h2d(h, db.data(), cb.data(), (int64_t)(n * sizeof(double))), "h2d");
    ddm_solve_result rr{};
    ddm_hip::check(h, ddm_fcg_solve(h, oh, ph, dx.data(), db.data(), 1e-10, 500, 3, complete, nullptr, &rr), "ddm_fcg_solve");
    ddm_hip::check(h, ddm_memcpy_d2h(h, cx.data(), dx.data(), (int64_t)(n * sizeof(double))), "d2h");
    ddm_hip::check(h, ddm_memcpy_d2h(h, cb.data(), db.data(), (int64_t)(n * sizeof(double))), "d2h");
    std::vector<double> ax(n), ab(n);
    for (std::size_t i = 0; i < n; ++i) { ax[i] = x1[i]; ab[i] = b1[i]; }
    const std::size_t dxn = differing(ax.data(), cx.data(), n), dbn = differing(ab.data(), cb.data(), n);
    std::printf("single %s %d %d %d %zu %zu\n", key, r1.iterations, rr.iterations, expected[0], dxn, dbn);
    ok = ok && r1.converged && rr.converged && r1.iterations == rr.iterations && r1.iterations == expected[0] && r1.iterations > 4 && r1.reduction == rr.reduction &&
         dxn == 0 && dbn == 0;
  }
  {
    std::vector<Dune::InverseOperatorResult> res;
    solver->apply(X, B, 1e-10, res);   // one upload, one block solve, one download
    ddm_hip::DeviceVector dX(ctx, n * m), dB(ctx, n * m);
    ddm_hip::check(h, ddm_memcpy_h2d(h, dX.data(), hx.data(), (int64_t)(n * m * sizeof(double))), "h2d");
    ddm_hip::check(h, ddm_memcpy_h2d(h, dB.data(), hb.data(), (int64_t)(n * m * sizeof(double))), "h2d");
    std::vector<ddm_solve_result> rr(m);
    ddm_hip::check(h, ddm_fcg_solve_multi(h, oh, ph, m, dX.data(), dB.data(), 1e-10, 500, 3, complete, nullptr, rr.data()), "ddm_fcg_solve_multi");
    ddm_hip::check(h, ddm_memcpy_d2h(h, hx.data(), dX.data(), (int64_t)(n * m * sizeof(double))), "d2h");
    ddm_hip::check(h, ddm_memcpy_d2h(h, hb.data(), dB.data(), (int64_t)(n * m * sizeof(double))), "d2h");
    ok = ok && res.size() == (std::size_t)m;
    for (int c = 0; c < m && ok; ++c) {
      std::size_t dxn = 0, dbn = 0;
      for (std::size_t i = 0; i < n; ++i) {
        const double xa = X[c][i], ba = B[c][i];
        dxn += std::memcmp(&xa, &hx[i * m + c], sizeof(double)) != 0;
        dbn += std::memcmp(&ba, &hb[i * m + c], sizeof(double)) != 0;
      }
      std::printf("col %s %d %d %d %d %zu %zu\n", key, c, res[c].iterations, rr[c].iterations, expected[1 + c], dxn, dbn);
      ok = ok && res[c].converged && rr[c].converged && res[c].iterations == rr[c].iterations && res[c].iterations == expected[1 + c] &&
           res[c].reduction == rr[c].reduction && dxn == 0 && dbn == 0;
    }
  }
  int threw = 0;
  try {   // there is no queued flexible CG loop
    std::vector<Vec> Bq = Bsave, Xq = zero_columns(n, m);
    std::vector<Dune::InverseOperatorResult> res;
    solver->apply_queue(Xq, Bq, 2, res);
  } catch (Dune::NotImplemented&) {
    threw = 1;
  }
  std::printf("queue %s %d\n", key, threw);
  return ok && threw == 1;
}

int main(int argc, char** argv)
{
  if (argc < 3) return 2;
  const std::string dir = argv[1];
  const int m = std::atoi(argv[2]);
  if (m < 1 || argc != 3 + 2 * (1 + m)) return 2;
  std::vector<int> expected;
  for (int a = 3; a < argc; ++a) expected.push_back(std::atoi(argv[a]));
  try {
    const Problem p = read_problem(dir);
    const auto bb = slurp<double>(dir + "/b.bin");
    bool ok = variant<Dune::HipRestartedFCGSolver<Vec>>("restartedfcgsolver", 0, p, bb, m, expected.data());
    ok = variant<Dune::HipCompleteFCGSolver<Vec>>("completefcgsolver", 1, p, bb, m, expected.data() + 1 + m) && ok;
    int caught = 0;
    try {   // an unknown key still throws, naming the six solvers
      const TwoLevel t = build_two_level(p, two_level_ptree("restricted", "ilu0", "multiplicative", "umfpack"));
      Dune::ParameterTree other;
      other["type"] = "minressolver";
      Dune::getHipSolver<Vec>(std::static_pointer_cast<Dune::LinearOperator<Vec, Vec>>(t.op), other, std::static_pointer_cast<Dune::Preconditioner<Vec, Vec>>(t.prec));
    } catch (Dune::NotImplemented& e) {
      const std::string w = e.what();
      if (w.find("restartedfcgsolver") != std::string::npos && w.find("completefcgsolver") != std::string::npos && w.find("restartedflexiblegmressolver") != std::string::npos) ++caught;
    }
    std::printf("errors_caught %d\n", caught);
    if (ok && caught == 1) std::printf("fcg_ok\n");
    return ok && caught == 1 ? 0 : 1;
  } catch (Dune::Exception& e) {
    std::cerr << "Dune exception: " << e.what() << "\n";
    return 1;
  }
}
