"""DP drivers: same module names as the reference's ``kmerpapa.algorithms`` (v0.2.4).

The two lattice-DP modules, the one-rate-per-k-mer model (``all_kmers_CV``)
and the greedy top-down heuristic (``greedy_penalty_plus_pseudo``) run on the GPU; BayesOpt
is out of scope (the reference's ``gp_minimize`` is unseeded).
"""
