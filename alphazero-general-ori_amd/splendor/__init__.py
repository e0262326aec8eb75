"""MI355X-native Splendor engine (HIP, gfx950) behind the reference's Game plug-in API.

Modules:
  _lib          ctypes binding of libsplendor_amd.so (fails loudly if missing)
  env           batched device-resident environment (SplendorEngine, RolloutBatch)
  SplendorGame  the reference's Game interface (SplendorGame.py:11-86), engine-backed
  SplendorPlayers  RandomPlayer / GreedyPlayer for the sequential Arena (one-board kernel calls)
  playout       PlayoutEvaluator: leaf values from random playouts (network-free search players
                and the rollout bootstrap of Coach.learn), safe under graph capture;
                MixedEvaluator: the network's priors, values mixed with the playouts'
  arena, pit    BatchedArena (the Coach's gate) and BatchedPit (any two player kinds), on device
"""
