"""Data constants of the speaker encoder (same names and values as DiffVC/speaker_encoder/encoder/params_data.py)."""
# mel filterbank
mel_window_length = 25      # ms
mel_window_step = 10        # ms
mel_n_channels = 40

# audio
sampling_rate = 16000
partials_n_frames = 160     # frames per partial utterance (1600 ms)
inference_n_frames = 80     # 800 ms

# voice activity detection
vad_window_length = 30      # ms; 10, 20 or 30
vad_moving_average_width = 8
vad_max_silence_length = 6

audio_norm_target_dBFS = -30
