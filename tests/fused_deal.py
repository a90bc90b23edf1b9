"""The tile dealing of k_verify_frames (csrc/hfv_frames_fused_kernel.hip) restated in plain Python,
and the sizes the dealing tests run it on.  Shared by test_frames_fused.py (CPU) and
test_gpu_frames_fused.py.

The launch has G = min(cap or CUs, ceil(T / W)) blocks for T = ceil(n / 64) tiles, W = 16 waves per
block under KEYSEL_ZERO and 12 under KEYSEL_IFID.  Block k owns the tiles [T*k/G, T*(k+1)/G); its LDS
counter starts at 0 and every claim (one per wave per round, in whatever order the waves arrive)
takes the next tile of the range; a wave whose claim lies past the range leaves."""

WAVES = {0: 16, 1: 12}          # keysel -> waves per block
CAPS = (1, 2, 3)                # hfv_debug_batch_grid values of the capped tests
REAL_GRID = 256                 # one block per CU of an MI355X
TILES_PER_WAVE = 5


def tiles_of(n):
    return (n + 63) // 64


def grid(n, keysel, cus=REAL_GRID, cap=0):
    w = WAVES[keysel]
    g = min(cus, (tiles_of(n) + w - 1) // w)
    if cap:
        g = min(g, cap)
    return max(g, 1)


def block_range(T, G, k):
    return T * k // G, T * (k + 1) // G


def claims(T, G, k, waves):
    """The tiles block k verifies, in claim order, and the number of claims its waves make in all
    (every wave's last claim is the one that finds the range used up)."""
    lo, hi = block_range(T, G, k)
    counter, taken = 0, []
    live = waves
    while live:
        t = lo + counter
        counter += 1
        if t >= hi:
            live -= 1
        else:
            taken.append(t)
    return taken, counter


def owners(n, keysel, cus=REAL_GRID, cap=0):
    """How often each tile of an n-frame call is verified: a list of T counts."""
    T, G = tiles_of(n), grid(n, keysel, cus, cap)
    seen = [0] * T
    for k in range(G):
        taken, total = claims(T, G, k, WAVES[keysel])
        assert total == len(taken) + WAVES[keysel]
        for t in taken:
            seen[t] += 1
    return seen


def deal_n(keysel, blocks):
    """Frames of a dealing test on `blocks` blocks: every wave claims TILES_PER_WAVE tiles or more on
    average, the block ranges are ragged (the tile count is no multiple of the block count for
    blocks > 1) and the last tile holds 37 frames."""
    return 64 * WAVES[keysel] * blocks * TILES_PER_WAVE + 37


# every n the GPU tests of test_gpu_frames_fused.py run (the dealing tests' sizes are added per keysel)
TEST_SIZES = (1, 63, 64, 65, 1000, 1025, 4001, 4096, 20000)
