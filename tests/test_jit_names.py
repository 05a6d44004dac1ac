"""Cache file names of the specialised XOR-network code objects (csrc/jit.hip,
api.hip jit_file).  A name is a key into files that travel between machines
(hbbft_amd/jit/), so it is pinned here as a literal: the stems are those of
the v23 objects, and only the version suffix moved (v24: the kernels lost
their p_only argument).  The retired A/B environment variables no longer
reach the names."""
import hbbft_amd as hb

V = "_v24.co"

# the BASELINE validator counts N = 4, 16, 64, 128, 250: (k, m) -> every group
ENCODERS = {
    (2, 2): ["hbrbc_enc_k2_m2_rt2_d4_r0_2_X"],
    (6, 10): ["hbrbc_enc_k6_m10_rt10_d4_r0_10_X"],
    (22, 42): ["hbrbc_enc_k22_m42_rt7_d4_r0_42_L_X_w4"],
    (44, 84): ["hbrbc_enc_k44_m84_rt6_d4_r0_48_L_w4",
               "hbrbc_enc_k44_m84_rt6_d4_r48_84_L_w4"],
    (84, 166): ["hbrbc_enc_k84_m166_rt6_d4_r0_48_L_X_w4",
                "hbrbc_enc_k84_m166_rt6_d4_r48_96_L_X_w4",
                "hbrbc_enc_k84_m166_rt6_d4_r96_144_L_X_w4",
                "hbrbc_enc_k84_m166_rt6_d4_r144_166_L_X_w4"],
}
# the shipped N = 250 decoder: only parity rows k..2k-1 present
DECODER = ["hbrbc_dec_n250_418319a74c63ef3b_rt6_d4_r0_48_L_w4",
           "hbrbc_dec_n250_418319a74c63ef3b_rt6_d4_r48_96_L_w4",
           "hbrbc_dec_n250_418319a74c63ef3b_rt6_d4_r96_144_L_w4",
           "hbrbc_dec_n250_418319a74c63ef3b_rt6_d4_r144_166_L_w4"]
# N = 64 in the plain chunk order
ENCODER_64_XCD0 = "hbrbc_enc_k22_m42_rt7_d4_r0_42_L_w4"


def check_names():
    for (k, m), stems in ENCODERS.items():
        got = [hb.jit_file_name(k, m, g) for g in range(hb.jit_encode_groups(k, m))]
        assert got == [s + V for s in stems]
    k, m = 84, 166
    present = [1 if k <= i < 2 * k else 0 for i in range(k + m)]
    for uf in (False, True):
        got = [hb.jit_decode_file_name(k, m, present, g, fused_unframe=uf)
               for g in range(hb.jit_decode_groups(k, m, present))]
        assert got == [s + ("_uf" if uf else "") + V for s in DECODER]


def test_code_object_names_are_pinned(monkeypatch):
    for var in ("HBRBC_JIT_XCD", "HBRBC_JIT_SPLIT", "HBRBC_RT_SPEC"):
        monkeypatch.delenv(var, raising=False)
    check_names()
    # retired switches change nothing
    monkeypatch.setenv("HBRBC_JIT_SPLIT", "0")
    monkeypatch.setenv("HBRBC_RT_SPEC", "8")
    check_names()
    # the chunk-order switch that stays drops the _X of every program
    monkeypatch.setenv("HBRBC_JIT_XCD", "0")
    assert hb.jit_file_name(22, 42, 0) == ENCODER_64_XCD0 + V
