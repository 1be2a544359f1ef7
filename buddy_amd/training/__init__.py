"""Training on the MI355X: the reference's ``Trainer`` surface over the HIP network and the fused clip + Adam + EMA step."""
