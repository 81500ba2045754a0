"""CPU: the comparator, the shape table and the tables' own shape of tests/engine_history.py (the GPU side: tests/test_gpu_engine_history.py)."""
import numpy as np
import pytest

import engine_history as H


# ---------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------
def test_comparator_passes_equal_finite_arrays():
    a = np.linspace(-3, 3, 24, dtype=np.float32).reshape(2, 3, 4)
    assert H.difference("a", a, a.copy()) is None
    assert H.differences({"a": a, "n": np.array([3, 4], dtype=np.int64)}, {"a": a.copy(), "n": np.array([3, 4], dtype=np.int64)}) == []


def test_comparator_reports_one_ulp():
    a = np.linspace(0.5, 3, 24, dtype=np.float32).reshape(4, 6)
    for toward in (np.float32(np.inf), np.float32(-np.inf)):
        b = a.copy()
        b[2, 5] = np.nextafter(b[2, 5], toward)
        assert np.allclose(a, b, rtol=2e-7, atol=0)        # (what a tolerance would let through)
        d = H.difference("a", a, b)
        assert d is not None and "1 of 24" in d and "(2, 5)" in d, d


def test_comparator_reports_the_sign_of_zero():
    a, b = np.zeros(5, dtype=np.float32), np.zeros(5, dtype=np.float32)
    b[3] = -0.0
    assert np.array_equal(a, b)
    d = H.difference("z", a, b)
    assert d is not None and "(3,)" in d, d
    assert H.difference("z", b, a) is not None


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_comparator_rejects_non_finite_on_either_side(bad):
    a = np.ones(6, dtype=np.float32)
    b = a.copy()
    b[1] = bad
    assert "twin" in H.difference("v", a, b)
    assert "worn" in H.difference("v", b, a)
    assert "non-finite" in H.difference("v", b, b.copy())       # the same NaN bits on both sides are still refused
    assert "non-finite" in H.difference("s", np.float32(bad), np.float32(bad))


def test_comparator_takes_zero_dimensional_records():
    """an optimizer's "step" entry is a 0-dim tensor"""
    assert H.difference("s", np.array(3.0, dtype=np.float32), np.array(3.0, dtype=np.float32)) is None
    d = H.difference("s", np.array(3.0, dtype=np.float32), np.array(2.0, dtype=np.float32))
    assert d is not None and "1 of 1" in d, d


def test_comparator_reports_shape_dtype_and_missing_records():
    a = np.ones((2, 3), dtype=np.float32)
    assert H.difference("a", a, a.reshape(3, 2)) is not None
    assert H.difference("a", a, a.astype(np.float64)) is not None
    assert len(H.differences({"a": a}, {"b": a})) == 2
    assert H.difference("n", np.array([1, 2]), np.array([1, 3])) is not None


# ---------------------------------------------------------------------------------------------
# the shape table: what each shape is claimed to wear
# ---------------------------------------------------------------------------------------------
def test_shape_table_properties():
    p, big, wide = H.shape_facts("probe"), H.shape_facts("BIG"), H.shape_facts("WIDE")
    assert (p["B"], p["T"]) == (3, 19) and p["N"] == 57 and p["n_mod16"] == 9 and p["pad8_n"] == 64
    assert p["panels"] == 2 and p["last_panel_rows"] == 25
    assert big["N"] == 280 and big["n_mod16"] == 8 and big["panels"] == 9 and big["last_panel_rows"] == 24
    assert big["pad8_t"] != p["pad8_t"]
    assert wide["batch_tiles32"] == 2 and wide["B"] % 32 == 1 and wide["len_ring_grows"] and not p["len_ring_grows"] and not big["len_ring_grows"]
    assert H.SHAPES["TINY_A"] == (1, 2) and H.SHAPES["TINY_B"] == (2, 1)


def test_every_padding_boundary_of_a_wear_shape_differs_from_the_probes():
    p = H.shape_facts("probe")
    for name in ("BIG", "WIDE", "TINY_A", "TINY_B"):
        f = H.shape_facts(name)
        for key in ("N", "n_mod16", "pad8_n", "panels", "last_panel_rows", "B", "T"):
            assert f[key] != p[key], (name, key, f[key])
    assert H.shape_facts("BIG")["N"] > p["N"] > H.shape_facts("TINY_A")["N"]       # shrink shrinks, grow grows
    assert H.shape_facts("WIDE")["N"] > p["N"]
    assert len(set(H.ABANDONED_T)) == 5 and H.FORWARD_SHAPE not in H.SHAPES.values()


# ---------------------------------------------------------------------------------------------
# the tables' own shape
# ---------------------------------------------------------------------------------------------
EXPECTED_BACKENDS = ["mlp_philox", "mlp_cond_split", "mlp_cond_cat", "mlp_cond_fused", "mlp_bf16", "mlp_adam_noR", "lstm_g", "lstm_steps",
                     "lstm_bf16", "lstm_d", "gru_g", "sru_g", "sru_bf16", "sru_d", "sru_d_bf16", "in2out", "in2out_rnn"]


def test_every_backend_names_an_existing_case():
    assert sorted(H.BACKENDS) == sorted(EXPECTED_BACKENDS)
    for name, b in H.BACKENDS.items():
        case = H.backend_case(name)
        assert case["update_d"] and case["update_g"] and case["adv_w"] > 0, name
        for opt, v in b["options"].items():
            assert v in H.OPTION_VALUES[opt], (name, opt, v)
    assert H.backend_case("mlp_adam_noR")["windows"] == 1 and H.backend_case("mlp_adam_noR")["opt_g"][0] == "Adam"
    assert H.backend_case("mlp_cond_split")["din"] % 4 != 0        # dense rows of x are not 16-byte pitched: the per-step copies are made
    for name in ("mlp_philox", "mlp_cond_split", "mlp_cond_cat", "mlp_cond_fused", "sru_g"):
        assert H.backend_case(name)["dropout_on"], name              # Philox on, nothing injected


def test_every_option_flip_names_an_option_with_two_values():
    from gantts_amd.engine import StepEngine
    import inspect
    known = inspect.getsource(StepEngine.set_option)
    for name, b in H.BACKENDS.items():
        opt, home, away = b["flip"]
        assert '"%s"' % opt in known, (name, opt)
        assert home != away and home in H.OPTION_VALUES[opt] and away in H.OPTION_VALUES[opt], (name, b["flip"])
        assert b["options"].get(opt, home) == home, (name, "the flip's home value is the one the backend runs with")
        if b["options"]:
            assert opt in b["options"], (name, "a backend with an option of its own flips that one")


def test_every_pair_of_the_tables_is_present_once():
    assert len(H.PAIRS) == len(set(H.PAIRS)) == 17 * 7 + 3 * 5
    assert set(h for _, h in H.PAIRS) == set(H.HISTORIES) == set(H.HISTORIES_ALL) | set(H.HISTORIES_FEW)
    for b in H.BACKENDS:
        assert [h for bb, h in H.PAIRS if bb == b][:7] == list(H.HISTORIES_ALL)
    assert set(b for b, h in H.PAIRS if h in H.HISTORIES_FEW) == set(H.BACKENDS_FEW)
    probe = H.SHAPES["probe"]
    for name, (shapes, wear) in H.HISTORIES.items():
        assert probe in shapes and callable(wear), name
    for b in H.BACKENDS_FEW:        # other_d: another kind, the same in_dim
        assert H.OTHER_D[H.backend_case(b)["d"]["kind"]]["kind"] != H.backend_case(b)["d"]["kind"]


def test_the_communicating_backends_have_a_table_and_a_pair_list_of_their_own():
    assert sorted(H.COMM_BACKENDS) == ["comm_cond_split", "comm_philox"] and not set(H.COMM_BACKENDS) & set(H.BACKENDS)
    assert H.COMM_BACKENDS["comm_cond_split"]["case"] == H.BACKENDS["mlp_cond_split"]["case"]       # split first layer: the count rides the gather
    assert H.COMM_BACKENDS["comm_philox"]["case"] == H.BACKENDS["mlp_philox"]["case"]               # split switched off: a launch of its own
    assert H.backend_case("comm_cond_split")["cond"] and not H.COMM_BACKENDS["comm_cond_split"]["options"]
    assert H.backend_case("comm_philox")["cond"] and H.COMM_BACKENDS["comm_philox"]["options"] == {"split_first_layer": 0}
    for name, b in H.COMM_BACKENDS.items():
        assert b["comm"] and b["flip"] == ("comm_tv_in_sums", 1, 0), name
        assert all(v in H.OPTION_VALUES["comm_tv_in_sums"] for v in b["flip"][1:])
    assert H.HISTORIES_COMM == ("same_shape_refill", "shrink", "poison_train_restore", "option_flip", "split_phase")
    assert len(H.COMM_PAIRS) == len(set(H.COMM_PAIRS)) == 10 and not set(H.COMM_PAIRS) & set(H.PAIRS)
    assert set(h for _, h in H.COMM_PAIRS) <= set(H.HISTORIES) and not any(b.get("comm") for b in H.BACKENDS.values())


EXPECTED_FEATURE_BACKENDS = ["wgan_clip", "hinge_fused", "ls_lstm_d", "sn_hinge", "sn_bce_bf16", "gp_r1", "gp_r1_fused", "gp_wgan_split", "gp_wgan_cat",
                             "ema_adagrad", "ema_adam", "all_wgan"]


def test_every_feature_backend_names_an_existing_case_that_fits_its_settings():
    from gantts_amd.engine import StepEngine
    import inspect
    known = inspect.getsource(StepEngine.set_option)
    assert list(H.FEATURE_BACKENDS) == EXPECTED_FEATURE_BACKENDS and not set(H.FEATURE_BACKENDS) & (set(H.BACKENDS) | set(H.COMM_BACKENDS))
    for name, b in H.FEATURE_BACKENDS.items():
        case, ft = H.backend_case(name), H.backend_features(name)
        assert case["update_d"] and case["update_g"] and case["adv_w"] > 0 and not b.get("comm"), name
        assert ft and set(b) <= {"case", "options", "flip"} | set(H.FEATURE_KEYS), name
        # the discriminator's last_sigmoid fits the objective (check_gan_objective refuses the bind otherwise)
        obj = ft.get("objective", "bce")
        assert obj in H.LAST_SIGMOID and bool(case["d"]["last_sigmoid"]) == H.LAST_SIGMOID[obj], (name, obj)
        if obj != "bce":
            assert H.LAST_SIGMOID[H.AWAY_OBJECTIVE[obj]] == H.LAST_SIGMOID[obj] and H.AWAY_OBJECTIVE[obj] != obj
        # the engine refuses penalty and spectral norm together, either of them on a recurrent discriminator, a penalty under bf16 products
        assert not (ft.get("grad_penalty") and ft.get("spectral_norm")), name
        if ft.get("grad_penalty") or ft.get("spectral_norm"):
            assert case["d"]["kind"] == "MLP", name
        if ft.get("grad_penalty"):
            assert ft["grad_penalty"][0] in ("r1", "wgan-gp") and ft["grad_penalty"][1] > 0 and not b["options"].get("matmul_bf16"), name
        if ft.get("ema_decay") is not None:
            assert 0.0 < ft["ema_decay"] < 1.0 and case["g"]["kind"] == "MLP", name
        # options and the flip, as for the old rows
        for opt, v in b["options"].items():
            assert v in H.OPTION_VALUES[opt], (name, opt, v)
        opt, home, away = b["flip"]
        assert '"%s"' % opt in known and home != away and home in H.OPTION_VALUES[opt] and away in H.OPTION_VALUES[opt], (name, b["flip"])
        assert b["options"].get(opt, home) == home and (opt in b["options"] if b["options"] else b["flip"] == ("launch_riders", 1, 0)), name
        assert case["dropout_on"] or name == "ema_adam", name          # Philox on, nothing injected
        assert case["din"] % 4 != 0 or name.startswith("ema_"), name    # dense rows of x are not 16-byte pitched: the per-step copies are made
    # the paths the rows were picked for
    fb, case_of = H.FEATURE_BACKENDS, H.backend_case
    assert case_of("hinge_fused")["d"]["hidden_dim"] == 128 == case_of("gp_r1_fused")["d"]["hidden_dim"]
    assert fb["hinge_fused"]["options"] == fb["gp_r1_fused"]["options"] == {"fused_dstack": 2}
    assert case_of("ls_lstm_d")["d"]["kind"] == "LSTMRNN"
    assert fb["sn_bce_bf16"]["options"] == {"matmul_bf16": 1} and "objective" not in fb["sn_bce_bf16"]
    assert case_of("gp_wgan_split")["cond"] and not fb["gp_wgan_split"]["options"] and fb["gp_wgan_cat"]["options"] == {"split_first_layer": 0}
    assert case_of("gp_wgan_cat") == case_of("gp_wgan_split") and case_of("gp_r1")["cond"] and case_of("sn_hinge")["cond"]
    assert case_of("ema_adagrad")["opt_g"][0] == "Adagrad" and case_of("ema_adam")["opt_g"][0] == "Adam"
    assert set(H.backend_features("all_wgan")) == {"objective", "weight_clip", "grad_penalty", "ema_decay"}
    # a bce row runs the reference's discriminator, every other one the case as it is
    import gan_objective_ref as G
    assert case_of("gp_r1") == G.bce_twin(G.STEP_CASES["mlp32_cond"]) and case_of("sn_hinge") == G.STEP_CASES["mlp32_cond"]


def test_the_feature_pairs_have_a_pair_list_of_their_own():
    FB = H.FEATURE_BACKENDS
    assert len(H.FEATURE_PAIRS) == len(set(H.FEATURE_PAIRS)) and not set(H.FEATURE_PAIRS) & (set(H.PAIRS) | set(H.COMM_PAIRS))
    assert set(b for b, _ in H.FEATURE_PAIRS) == set(FB)
    for b in FB:          # every row runs the seven histories of the old rows
        assert [h for bb, h in H.FEATURE_PAIRS if bb == b][:7] == list(H.HISTORIES_ALL)

    def rows_of(history):
        return sorted(b for b, h in H.FEATURE_PAIRS if h == history)
    gp = sorted(b for b in FB if FB[b].get("grad_penalty"))
    assert gp == sorted(["gp_r1", "gp_r1_fused", "gp_wgan_split", "gp_wgan_cat", "all_wgan"]) == rows_of("gp_hooks")
    assert rows_of("feature_off_and_on") == sorted(set(gp) | {"wgan_clip", "hinge_fused", "ls_lstm_d", "sn_hinge"})
    assert rows_of("sn_other_d") == ["sn_bce_bf16", "sn_hinge"] == sorted(b for b in FB if FB[b].get("spectral_norm"))
    assert rows_of("ema_swap_and_roles") == ["all_wgan", "ema_adagrad", "ema_adam"] == sorted(b for b in FB if "ema_decay" in FB[b])
    for h in ("phase_and_roles", "abandoned_passes", "split_phase"):
        assert rows_of(h) == ["ema_adam", "gp_wgan_split", "sn_hinge"], h
    assert rows_of("normaliser") == ["gp_wgan_split"] and rows_of("shard_and_normaliser") == ["ema_adam", "sn_hinge"]
    assert len(H.FEATURE_PAIRS) == 12 * 7 + 9 + 5 + 2 + 3 + 3 * 3 + 3
    # every history of a feature pair exists, lists the probe shape and, where it steps at BIG, that one too
    probe = H.SHAPES["probe"]
    assert not set(H.FEATURE_HISTORIES) & (set(H.HISTORIES) - {"shard_and_normaliser"})
    for name in set(h for _, h in H.FEATURE_PAIRS):
        shapes, wear = H.feature_history(name)
        assert probe in shapes and callable(wear), name
    for name, (shapes, wear) in H.FEATURE_HISTORIES.items():
        assert probe in shapes and H.SHAPES["BIG"] in shapes and callable(wear), name
    assert H.feature_history("shard_and_normaliser")[1] is not H.HISTORIES["shard_and_normaliser"][1]      # (it asserts the refusal under spectral norm)
    # the old tables are what they were
    assert len(H.PAIRS) == 17 * 7 + 3 * 5 and len(H.COMM_PAIRS) == 10
    assert set(H.ALL_BACKENDS) == set(H.BACKENDS) | set(H.COMM_BACKENDS) | set(FB)


def test_batches_are_cached_per_shape_and_poison_covers_the_valid_frames():
    a, b = H.shape_batch("mlp_cond_split", "BIG", 1), H.shape_batch("mlp_cond_split", "BIG", 1)
    assert a is b and not a["x"].flags.writeable
    p = H.shape_batch("mlp_cond_split", "BIG", 1, poison=True)
    valid = np.arange(p["T"])[None, :] < p["lengths"][:, None]
    assert np.isnan(p["x"][valid]).all() and np.isnan(p["y"][valid]).all()
    assert np.isfinite(p["x"][~valid]).all() and (~valid).any() and int(p["lengths"].max()) == p["T"]
    assert not np.array_equal(H.shape_batch("mlp_cond_split", "probe", 1)["x"], H.shape_batch("mlp_cond_split", "probe", 2)["x"])
