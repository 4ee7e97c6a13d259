"""The rounding window around the kink of ReLU / LeakyReLU.

The derivative of ReLU / LeakyReLU is discontinuous at 0.  The product associates its sums differently from the oracle
(project-then-gather, folded first Linear), so a pre-activation that lies within fp32 rounding of zero may take the other
derivative branch -- about one activation in 10^5 at tau = 1e-5.  Gradient tests make no exception for such units: the
oracle is pinned to the branches the product took (``dmp_oracle.PIN``, tests/util_branches.py), and ``TAU`` bounds where
those branches may differ from the oracle's own -- a branch that differs outside the window is an error."""

TAU = 1e-5          # |pre-activation| <= TAU * max(1, |pre|max): "within rounding of the kink"
