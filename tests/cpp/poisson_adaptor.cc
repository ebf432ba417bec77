// Drives the DUNE-facing adaptors (dune-ddm_amd/dune/ddm/hip/*.hh) the way examples/poisson.cc:229-321
// drives the reference classes: SchwarzPreconditioner + (POU) GalerkinPreconditioner +
// CombinedPreconditioner + NonOverlappingOperator + its scalar product inside a CG loop written
// against the abstract dune-istl interfaces.  Single rank (mock communication, see mock/).
//   usage: poisson_adaptor <dir with n.txt rowptr.bin col.bin val.bin b.bin dirichlet.bin pou.bin> <mode>
// mode = additive | multiplicative : dune-istl's CG written out on the abstract interfaces (two PCIe copies per virtual call)
// mode = device | device_cholmod   : the factory-style path -- coarse space from a CoarseSpaceBuilder task, solver from
//                                    Dune::getHipSolver (whole CG on the device: one upload, one download), subdomain solver
//                                    ilu0 resp. cholmod; also exercises the Dune::InverseOperator plugin HipSubdomainSolver
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "adaptor_fixture.hh"   // first: the adaptor headers below expect the dune-istl ones before them

#include <dune/ddm/hip/solvers.hh>
#include <dune/ddm/hip/rccl_exchange.hh>

int main(int argc, char** argv)
{
  if (argc < 3) return 2;
  const std::string dir = argv[1], mode = argv[2];
  try {
    if (std::getenv("DDM_TEST_RCCL")) {   // the in-library RCCL exchange installed the way a DUNE program would (size-1 communicator, self test)
      auto ctx = ddm_hip::install_rccl_exchange(ddm_hip::make_rccl_id(), 0, 1, 0, /*self_test=*/true);
      std::printf("rccl_exchange installed rank %d of %d\n", ctx->rank, ctx->nranks);
      try { ddm_hip::install_rccl_exchange(ddm_hip::RcclId(), 2, 1); } catch (Dune::InvalidStateException&) { std::printf("rccl_bad_rank_caught\n"); }
    }
    const Problem problem = read_problem(dir);
    const auto& [n, A, comm, dm, pw] = problem;
    const auto bb = slurp<double>(dir + "/b.bin");
    const bool device = mode.rfind("device", 0) == 0, cholmod = mode == "device_cholmod";
    const auto ptree = two_level_ptree("standard", cholmod ? "cholmod" : "ilu0", device ? "additive" : mode, cholmod ? "cholmod" : "umfpack");
    if (device) {
      const TwoLevel t = build_two_level(problem, ptree);   // examples/poisson.cc:229-321 with the device-resident pieces
      Dune::ParameterTree solver_subtree;
      solver_subtree["type"] = "cgsolver";
      solver_subtree["reduction"] = "1e-10";
      solver_subtree["maxit"] = "500";
      auto solver = Dune::getHipSolver<Vec>(t.op, solver_subtree, t.prec);
      Dune::InverseOperatorResult res;
      Vec v(n), b = to_vec(bb);
      v = 0;
      solver->apply(v, b, res);   // poisson.cc:318-319
      std::printf("device_solve iterations %d converged %d reduction %.17g\n", res.iterations, (int)res.converged, res.reduction);
      write_bin(dir + "/x_device.bin", v);
      // the InverseOperator plugin on its own: exact solve A y = b with the sparse Cholesky, ILU(0) application
      Dune::HipSubdomainSolver<Mat> chol(*A, "cholesky"), ilu(*A, "ilu0");
      Vec y(n), rhs = to_vec(bb), z(n);
      Dune::InverseOperatorResult r2;
      chol.apply(y, rhs, r2);
      double rmax = 0, bmax = 0;
      for (auto ri = A->begin(); ri != A->end(); ++ri) {
        double s = 0;
        for (auto c = ri->begin(); c != ri->end(); ++c) s += (*c)[0][0] * y[c.index()][0];
        rmax = std::max(rmax, std::fabs(s - bb[ri.index()]));
        bmax = std::max(bmax, std::fabs(bb[ri.index()]));
      }
      ilu.apply(z, rhs, r2);
      std::printf("plugin cholesky_residual %.3e converged %d\n", rmax / bmax, (int)r2.converged);
      int caught = 0;
      try { Dune::HipSubdomainSolver<Mat> bad(*A, "bogus"); } catch (Dune::NotImplemented&) { ++caught; }
      try { solver_subtree["type"] = "minressolver"; Dune::getHipSolver<Vec>(t.op, solver_subtree, t.prec); } catch (Dune::NotImplemented&) { ++caught; }
      std::printf("errors_caught %d\n", caught);
      return 0;
    }

    auto pou = std::make_shared<PartitionOfUnity>(pw);
    auto schwarz = std::make_shared<SchwarzPreconditioner<Mat, Vec, Comm>>(A, comm, pou, ptree);
    // POUCoarseSpace + zero_at_dirichlet (coarse_spaces.hh:1211-1224, poisson.cc:235-238)
    std::vector<Vec> basis(1, Vec(n));
    double nrm = 0;
    for (std::size_t i = 0; i < n; ++i) nrm += pw[i] * pw[i];
    for (std::size_t i = 0; i < n; ++i) basis[0][i] = dm[i] ? 0.0 : pw[i] / std::sqrt(nrm);
    auto coarse = std::make_shared<GalerkinPreconditioner<Vec, Comm>>(*A, basis, comm, ptree, "coarse_solver");
    auto op = std::make_shared<NonOverlappingOperator<Mat, Vec, Vec, Comm>>(A, comm);
    auto prec = std::make_shared<CombinedPreconditioner<Vec>>(ptree);
    prec->set_op(op);
    prec->add(schwarz);
    prec->add(coarse);
    auto sp = Dune::createScalarProduct(op);

    // dune-istl CGSolver::apply on the abstract interfaces
    Dune::LinearOperator<Vec, Vec>& L = *op;
    Dune::Preconditioner<Vec, Vec>& P = *prec;
    Vec x(n), b(n), p(n), q(n);
    x = 0;
    for (std::size_t i = 0; i < n; ++i) b[i] = bb[i];
    P.pre(x, b);
    L.applyscaleadd(-1.0, x, b);
    const double def0 = sp->norm(b);
    std::printf("it 0 %.17g\n", def0);
    p = 0;
    P.apply(p, b);
    double rholast = sp->dot(p, b);
    for (int i = 1; i <= 500; ++i) {
      L.apply(p, q);
      const double lambda = rholast / sp->dot(p, q);
      x.axpy(lambda, p);
      b.axpy(-lambda, q);
      const double def = sp->norm(b);
      std::printf("it %d %.17g\n", i, def);
      if (def < def0 * 1e-10) break;
      q = 0;
      P.apply(q, b);
      const double rho = sp->dot(q, b);
      p *= rho / rholast;
      p += q;
      rholast = rho;
    }
    P.post(x);
    std::printf("coarse %d %.17g\n", coarse->coarse_size(), coarse->coarse_matrix()[0]);
    // error conventions: unknown Schwarz type / missing solver key throw like the reference
    int caught = 0;
    try {
      Dune::ParameterTree bad;
      bad.sub("schwarz")["type"] = "bogus";
      bad.sub("schwarz").sub("subdomain_solver")["type"] = "ilu0";
      SchwarzPreconditioner<Mat, Vec, Comm> s(A, comm, pou, bad);
    } catch (Dune::NotImplemented&) { ++caught; }
    try {
      Dune::ParameterTree bad;
      SchwarzPreconditioner<Mat, Vec, Comm> s(A, comm, pou, bad);
    } catch (Dune::Exception&) { ++caught; }
    try {
      Dune::ParameterTree bad;
      bad.sub("combined_preconditioner")["mode"] = "bogus";
      CombinedPreconditioner<Vec> c(bad);
    } catch (Dune::NotImplemented&) { ++caught; }
    // coarse solver key (galerkin_preconditioner.hh:338-346): missing -> Dune::Exception, iterative factory entry -> NotImplemented
    try {
      Dune::ParameterTree bad;
      GalerkinPreconditioner<Vec, Comm> g(*A, basis, comm, bad, "coarse_solver");
    } catch (Dune::NotImplemented&) {
    } catch (Dune::Exception& e) { if (std::string(e.what()).find("using the key 'type'") != std::string::npos) ++caught; }
    try {
      Dune::ParameterTree bad;
      bad.sub("coarse_solver")["type"] = "cgsolver";
      GalerkinPreconditioner<Vec, Comm> g(*A, basis, comm, bad, "coarse_solver");
    } catch (Dune::NotImplemented&) { ++caught; }
    // getSolver() (schwarz.hh:155): the local solver as an InverseOperator on the overlapping index set; ILU(0) here, so
    // check it against the factor the library exposes: L U x = b  <=>  residual of the incomplete factorisation is not zero,
    // but applying it twice to the same right-hand side must give the same result and a finite, non-trivial vector
    {
      auto& ls = schwarz->getSolver();
      Vec xa(n), xb(n), rhs(n);
      for (std::size_t i = 0; i < n; ++i) rhs[i] = bb[i];
      Dune::InverseOperatorResult r1;
      ls.apply(xa, rhs, r1);
      for (std::size_t i = 0; i < n; ++i) rhs[i] = bb[i];
      ls.apply(xb, rhs, r1);
      double diff = 0, nrm = 0;
      for (std::size_t i = 0; i < n; ++i) { diff = std::max(diff, std::fabs(xa[i][0] - xb[i][0])); nrm = std::max(nrm, std::fabs(xa[i][0])); }
      // and against the preconditioner itself: on one rank with pou == 1 on all owner indices, Schwarz::apply IS the local solve
      Vec xs(n);
      schwarz->apply(xs, rhs);
      double dev = 0;
      for (std::size_t i = 0; i < n; ++i) dev = std::max(dev, std::fabs(xs[i][0] - xa[i][0]));
      std::printf("getSolver repeat_diff %.3e vs_apply %.3e norm %.3e converged %d\n", diff, dev, nrm, (int)r1.converged);
    }
    std::printf("errors_caught %d\n", caught);
  } catch (Dune::Exception& e) {
    std::cerr << "Dune exception: " << e.what() << "\n";
    return 1;
  }
  return 0;
}
