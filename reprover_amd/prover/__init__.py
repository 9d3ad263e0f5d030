"""Mirror of the reference's ``prover/`` package: the tactic generators of proof search."""
